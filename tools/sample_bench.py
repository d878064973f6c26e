"""Token-choice kernel timing (profiles/r9/sample_filtered.txt): hpa_sample_final (the order-exact reference
sampler) against hpa_sample_filtered at five settings, B x 50257 'randn3' logits (tests/test_gpu_sampling.py),
B = 8 and 64, HIP events around back-to-back launches.  Usage: python tools/sample_bench.py [out.txt]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm.c-paged_amd"))
import numpy as np  # noqa: E402
import pagedattn as pa  # noqa: E402

pa.init(0)
L = pa.lib()
V, WARM, ITERS, ROUNDS = 50257, 20, 1000, 5
SETTINGS = [("T=1   k=0  P=1  ", 1.0, 0, 1.0), ("T=0.8 k=50 P=1  ", 0.8, 50, 1.0), ("T=0.8 k=0  P=0.9", 0.8, 0, 0.9),
            ("T=0.8 k=50 P=0.9", 0.8, 50, 0.9), ("all greedy (T=0)", 0.0, 0, 1.0)]
lines = [f"token-choice kernels, {pa.device_info()[0]}",
         f"logits: B x {V} fp32, randn * 3 (seed 3), resident in device memory; one launch draws one token per row",
         f"time: HIP events around {ITERS} back-to-back launches on one stream after {WARM} warm-up launches;",
         f"{ROUNDS} rounds, the variants alternating inside every round; us per launch: median [min .. max]",
         "spread = max - min of a variant's rounds; 'no slower' = filtered median <= baseline median + both spreads", ""]
e0, e1 = L.hpa_event_create(), L.hpa_event_create()
for B in (8, 64):
    x = (np.random.default_rng(3).standard_normal((B, V)) * 3).astype(np.float32)
    d_x = pa.DeviceBuffer.from_array(x)
    d_st = pa.DeviceBuffer.from_array(np.arange(B, dtype=np.uint64) + np.uint64(1337))
    d_next = pa.DeviceBuffer(B * 4)
    d_k = pa.DeviceBuffer(B * 4)
    d_t, d_p = pa.DeviceBuffer(B * 4), pa.DeviceBuffer(B * 4)

    def baseline():
        pa.check(L.hpa_sample_final(d_x.ptr, B, V, d_st.ptr, d_next.ptr, None, None, None))

    def filtered():
        pa.check(L.hpa_sample_filtered(d_x.ptr, B, V, d_t.ptr, d_k.ptr, d_p.ptr, d_st.ptr, d_next.ptr, None, None,
                                       None, None, None))

    variants = [("hpa_sample_final (baseline)  ", baseline, None)]
    variants += [("hpa_sample_filtered " + n, filtered, (t, k, p)) for n, t, k, p in SETTINGS]
    us = {n: [] for n, _, _ in variants}
    for r in range(ROUNDS):
        for name, fn, par in variants:
            if par:
                d_t.upload(np.full(B, par[0], np.float32))
                d_k.upload(np.full(B, par[1], np.int32))
                d_p.upload(np.full(B, par[2], np.float32))
            for _ in range(WARM):
                fn()
            pa.check(L.hpa_event_record(e0))
            for _ in range(ITERS):
                fn()
            pa.check(L.hpa_event_record(e1))
            us[name].append(L.hpa_event_elapsed_ms(e0, e1) * 1e3 / ITERS)
    base = us[variants[0][0]]
    bmed, bspread = float(np.median(base)), max(base) - min(base)
    lines.append(f"B = {B}")
    for name, _, par in variants:
        v = us[name]
        med, spread = float(np.median(v)), max(v) - min(v)
        note = ""
        if par:
            ok = med <= bmed + bspread + spread
            note = f"  {bmed / med:5.2f}x the baseline's rate, {'no slower' if ok else 'SLOWER'}"
        lines.append(f"  {name}: {med:8.2f} [{min(v):8.2f} .. {max(v):8.2f}] us{note}")
    lines.append("")
out = "\n".join(lines)
print(out)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(out)
