#!/usr/bin/env python3
"""Prefill attention on fp32 KV pools at GPT-2 124M shapes (12 heads, page 16):
hpa_paged_attention_prefill_split (the bf16 matrix pipe on split operands)
against hpa_paged_attention_prefill_ragged (prefill_attn_kernel: the default
route), on the same pool, tables and queries.  HIP events around a few
back-to-back launches, five samples after a discarded warm-up, the two kernels
alternating in one process: median us per launch and the spread max - min.
Each shape also prints the largest difference between the two outputs, relative
to the largest output.  Shapes: B = 8 and 64 with T = 988 rows from start 0; a
chunk of T = 256 at start 768; T = 8 at start 1000 (the verify shape).
Then one whole prefill_ragged pass (wall clock: the call is host-synchronous)
under request 3 and request 0 on the same engine: fp32 weights and bf16
weights, both on the fp32 pool, B = 8, 988 tokens per sequence.
usage: prefill_split_scan.py [--passes 5] [--kernels-only]
HPA_LIB=<path> runs another build of the library."""
import argparse
import ctypes
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm.c-paged_amd"))
import numpy as np  # noqa: E402
import pagedattn as pa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--kernels-only", action="store_true", help="skip the whole-pass timings")
args = ap.parse_args()

NH, HS, P, MAXC, REPEATS = 12, 64, 16, 1024, 5
C = NH * HS
_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
SHAPES = ((8, 988, 0), (64, 988, 0), (8, 256, 768), (64, 256, 768), (8, 8, 1000), (64, 8, 1000))  # B, T, start

pa.init(0)
L = pa.lib()
print(f"# {pa.device_info()[0].strip()}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# GPT-2 124M heads, fp32 pool, page {P}; {REPEATS} samples, the kernels alternating: median us per launch (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)


def med(v):
    return statistics.median(v), max(v) - min(v)


def cast(buf, ty):
    return ctypes.cast(buf.ptr, ty)


npg = MAXC // P
pool = pa.Pool(1, NH, P, 64 * npg, dtype=pa.HPA_F32)
tables = rng.permutation(64 * npg).astype(np.int32).reshape(64, npg)
d_bt = pa.DeviceBuffer.from_array(tables)
pa.check(L.hpa_pool_fill_random(pool.ref, d_bt.ptr, npg, 64, MAXC, 7), "fill")
fns = {"split": L.hpa_paged_attention_prefill_split, "prefill": L.hpa_paged_attention_prefill_ragged}
for B, T, start in SHAPES:
    R = B * T
    launches = 3 if R > 20000 else 20
    d_q = pa.DeviceBuffer.from_array(rng.uniform(-1, 1, (R, C)).astype(np.float32))
    d_start = pa.DeviceBuffer.from_array(np.full(B, start, np.int32))
    d_out = {k: pa.DeviceBuffer((R + 15) // 16 * 16 * C * 4) for k in fns}

    def run(k):
        pa.check(fns[k](cast(d_q, _F), pool.ref, 0, cast(d_bt, _I), npg, cast(d_start, _I), None, None, B, T,
                        cast(d_out[k], _F)), k)

    def sample(k):
        t.start()
        for _ in range(launches):
            run(k)
        return t.stop() * 1e3 / launches

    for k in fns:  # warm-up: code objects, clocks
        run(k)
        run(k)
    pa.check(L.hpa_synchronize())
    o = {k: d_out[k].download(R * C) for k in fns}  # whole 16-row blocks where R % 16 == 0 (every shape here)
    diff = float(np.abs(o["split"] - o["prefill"]).max() / np.abs(o["prefill"]).max())
    got = {k: [] for k in fns}
    for i in range(REPEATS + 1):  # sample 0 is discarded
        for k in fns:
            x = sample(k)
            if i:
                got[k].append(x)
    m = {k: med(v) for k, v in got.items()}
    gap = m["prefill"][0] - m["split"][0]
    verdict = "wins" if gap > max(m["prefill"][1], m["split"][1]) else \
        "loses" if -gap > max(m["prefill"][1], m["split"][1]) else "within the spreads"
    print(f"f32 B={B:3d} T={T:4d} start={start:4d}: " + "   ".join(f"{k} {v[0]:9.2f} ({v[1]:7.2f})" for k, v in m.items())
          + f"   prefill / split {m['prefill'][0] / m['split'][0]:5.2f}   split {verdict}   max |diff| / max |out| {diff:.2e}",
          flush=True)
    for k, v in got.items():
        print(f"    repeats {k:8s}{' '.join(f'{x:.2f}' for x in v)}")
    for b in [d_q, d_start, *d_out.values()]:
        b.free()
d_bt.free()
del pool

# ---- whole prefill_ragged passes, request 3 against request 0 on one engine
B, T = 8, 988
for name, kw in (() if args.kernels_only else (("fp32 weights / fp32 pool", dict(kv_dtype=pa.HPA_F32)),
                                               ("bf16 weights / fp32 pool", dict(kv_dtype=pa.HPA_F32, w_dtype=pa.HPA_BF16)))):
    m = pa.Model(dict(pa.GPT2_124M), seed=1)
    m.decode_init(B, P, MAXC, **kw)
    seqs = [rng.integers(0, 50257, T).astype(np.int32) for _ in range(B)]
    zero = np.zeros(B, np.int32)

    def pass_ms(request):
        m.set_prefill_attention(request)
        total = 0.0
        for i in range(args.passes + 1):  # the first pass of a sample is its warm-up
            m.set_positions(zero)
            t0 = time.perf_counter()
            m.prefill_ragged(seqs)
            if i:
                total += (time.perf_counter() - t0) * 1e3
        return total / args.passes

    got = {3: [], 0: []}
    for _ in range(REPEATS):
        for rq in got:
            got[rq].append(pass_ms(rq))
    md = {k: med(v) for k, v in got.items()}
    print(f"{name} B={B} T={T}: prefill_ragged pass " + "   ".join(f"request {k}: {v[0]:8.3f} ms ({v[1]:6.3f})" for k, v in md.items())
          + f"   request 0 / request 3 {md[0][0] / md[3][0]:5.2f}", flush=True)
    for k, v in got.items():
        print(f"    repeats request {k}  {' '.join(f'{x:.3f}' for x in v)}")
    m.close()
