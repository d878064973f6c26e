#!/usr/bin/env python3
"""The attention of a speculative verify pass on bf16 and fp8 KV pools at GPT-2
124M shapes (12 heads, page 16, the last row's context 1000), B = 64 and B = 8,
2, 4 and 8 query rows per sequence.  HIP events around 20 back-to-back
launches, five repeats, the versions alternating in one process (median per
launch, and the spread max - min):
  * packed:  hpa_paged_attention_verify_packed, chain form, the library's pick
             of the decode placement;
  * form a / form b: the same with hpa_set_verify_packed_form(1) / (2) -- codes
             decoded inside each row's loop / once per tile;
  * tree:    the tree form with chain masks (the same visible keys);
  * prefill: hpa_paged_attention_prefill_ragged on the same pool and tables --
             the only route the parent commit has;
  * decode:  one hpa_paged_attention_decode launch on the same pool: the floor
             for reading the same K/V once.
Consecutive launches walk over 64 / B copies of the batch in different pages,
so every launch streams from HBM.
Then whole gpt2_decode_verify passes of 4 and 8 rows per sequence (wall clock:
the call is host-synchronous) under request 3 and request 0 on the same
engine, against its graph-replayed decode step, with the break-even number of
accepted drafts per pass (pass / step - 1).
usage: verify_packed_scan.py [--steps 200]
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
ap.add_argument("--steps", type=int, default=200)
args = ap.parse_args()

NH, HS, P, CTX, REPEATS, LAUNCHES = 12, 64, 16, 1000, 5, 20
C = NH * HS
_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
_U8 = ctypes.POINTER(ctypes.c_ubyte)

pa.init(0)
L = pa.lib()
ncu = pa.device_info()[1]
print(f"# {pa.device_info()[0].strip()}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# GPT-2 124M heads, page {P}, ctx {CTX}; {LAUNCHES} launches per sample, {REPEATS} samples: "
      f"median us per launch (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)


def med(v):
    return statistics.median(v), max(v) - min(v)


def cast(buf, ty):
    return ctypes.cast(buf.ptr, ty)


for name, dtype in (("bf16", pa.HPA_BF16), ("fp8", pa.HPA_FP8)):
    for B in (64, 8):
        nsets = max(1, 64 // B)
        npg = (CTX + P - 1) // P
        pool = pa.Pool(1, NH, P, nsets * B * npg, dtype=dtype)
        tables = rng.permutation(nsets * B * npg).astype(np.int32).reshape(nsets, B, npg)
        d_bt = [pa.DeviceBuffer.from_array(np.ascontiguousarray(tables[s])) for s in range(nsets)]
        for s in range(nsets):
            pa.check(L.hpa_pool_fill_random(pool.ref, d_bt[s].ptr, npg, B, CTX, 7 + s), "fill")
        waves = L.hpa_attn_pick_waves(B, NH, 1, ncu)
        d_pos = pa.DeviceBuffer.from_array(np.full(B, CTX - 1, np.int32))
        d_q1 = pa.DeviceBuffer.from_array(rng.uniform(-1, 1, (B, C)).astype(np.float32))
        d_o1 = pa.DeviceBuffer((B + 15) // 16 * 16 * C * 4)
        for rows in (2, 4, 8):
            R = B * rows
            d_q = pa.DeviceBuffer.from_array(rng.uniform(-1, 1, (R, C)).astype(np.float32))
            d_out = pa.DeviceBuffer((R + 15) // 16 * 16 * C * 4)
            d_start = pa.DeviceBuffer.from_array(np.full(B, CTX - rows, np.int32))
            d_row0 = pa.DeviceBuffer.from_array((np.arange(B) * rows).astype(np.int32))
            d_len = pa.DeviceBuffer.from_array(np.full(B, rows, np.int32))
            d_anc = pa.DeviceBuffer.from_array(np.tile((2 << np.arange(rows)) - 1, B).astype(np.uint8))

            def packed(form, anc):
                def run(i):
                    pa.check(L.hpa_set_verify_packed_form(form))
                    pa.check(L.hpa_paged_attention_verify_packed(
                        cast(d_q, _F), pool.ref, 0, cast(d_bt[i % nsets], _I), npg, cast(d_start, _I), cast(d_row0, _I),
                        cast(d_len, _I), cast(d_anc, _U8) if anc else None, B, rows, cast(d_out, _F)), "packed")
                return run

            def prefill(i):
                pa.check(L.hpa_paged_attention_prefill_ragged(
                    cast(d_q, _F), pool.ref, 0, cast(d_bt[i % nsets], _I), npg, cast(d_start, _I), cast(d_row0, _I),
                    cast(d_len, _I), B, rows, cast(d_out, _F)), "prefill")

            def decode(i):
                pa.check(L.hpa_paged_attention_decode_split_w(d_q1.ptr, pool.ref, 0, d_bt[i % nsets].ptr, npg,
                                                              d_pos.ptr, d_o1.ptr, B, 1, None, 1, waves), "decode")

            def sample(fn):
                t.start()
                for i in range(LAUNCHES):
                    fn(i)
                return t.stop() * 1e3 / LAUNCHES

            fns = {"packed": packed(0, False), "form a": packed(1, False), "form b": packed(2, False),
                   "tree": packed(0, True), "prefill": prefill, "decode": decode}
            got = {k: [] for k in fns}
            try:  # the form is a process-wide switch: the library's pick is back however this ends
                for fn in fns.values():  # warm-up: code objects, clocks
                    for i in range(4):
                        fn(i)
                pa.check(L.hpa_synchronize())
                for _ in range(REPEATS):
                    for k, fn in fns.items():
                        got[k].append(sample(fn))
            finally:
                pa.check(L.hpa_set_verify_packed_form(0))
            m = {k: med(v) for k, v in got.items()}
            wins = m["prefill"][0] - m["packed"][0] > max(m["prefill"][1], m["packed"][1])
            print(f"{name} B={B:3d} rows={rows}: " + "   ".join(f"{k} {v[0]:7.2f} ({v[1]:5.2f})" for k, v in m.items())
                  + f"   prefill / packed {m['prefill'][0] / m['packed'][0]:5.2f}   packed / decode "
                  f"{m['packed'][0] / m['decode'][0]:4.2f}   packed {'wins' if wins else 'does not win'}", flush=True)
            for k, v in got.items():
                print(f"    repeats {k:8s}{' '.join(f'{x:.2f}' for x in v)}")
            for b in (d_q, d_out, d_start, d_row0, d_len, d_anc):
                b.free()
        for b in d_bt + [d_pos, d_q1, d_o1]:
            b.free()
        del pool

# ---- whole verify passes of 4 and 8 rows against the graph-replayed decode step
MAXC, WIN = 1024, 20
FILL = MAXC - 8 - WIN
for name, kw in (("bf16", dict(kv_dtype=pa.HPA_BF16, w_dtype=pa.HPA_BF16)), ("fp8", dict(kv_dtype=pa.HPA_FP8))):
    for B in (64, 8):
        m = pa.Model(dict(pa.GPT2_124M), seed=1)
        m.decode_init(B, P, MAXC, **kw)
        m.fill_random(FILL, seed=3)
        m.set_graph(True)
        m.step(np.zeros(B, np.int32))  # a valid pending id per sequence
        pos = np.full(B, FILL, np.int32)

        def step_ms():
            m.set_positions(pos)
            for _ in range(WIN):
                m.step_async()
            total, n = 0.0, 0
            while n < args.steps:
                m.set_positions(pos)
                t.start()
                for _ in range(WIN):
                    m.step_async()
                total += t.stop()
                n += WIN
            m.status()
            return total / n

        def pass_ms(request, rows):
            drafts = [list(range(1, rows))] * B
            m.set_verify_attention(request)
            for _ in range(3):
                m.set_positions(pos)
                m.verify(drafts)
            total, n = 0.0, 0
            while n < max(20, args.steps // 10):
                m.set_positions(pos)
                t0 = time.perf_counter()
                m.verify(drafts)
                total += (time.perf_counter() - t0) * 1e3
                n += 1
            return total / n

        keys = [("step", None)] + [(f"{rows} rows request {rq}", (rq, rows)) for rows in (4, 8) for rq in (3, 0)]
        got = {k: [] for k, _ in keys}
        for _ in range(REPEATS):
            for k, a in keys:
                got[k].append(step_ms() if a is None else pass_ms(*a))
        md = {k: med(v) for k, v in got.items()}
        sm = md["step"][0]
        print(f"{name} B={B:3d} ctx~{FILL}: decode step (graph, form {m.layer_form()}) {sm:7.4f} ms ({md['step'][1]:6.4f})   "
              + "   ".join(f"{k}: {v[0]:7.4f} ms ({v[1]:6.4f}), break-even {v[0] / sm - 1:4.2f} accepted"
                           for k, v in md.items() if k != "step"), flush=True)
        for k, v in got.items():
            print(f"    repeats {k:18s}{' '.join(f'{x:.4f}' for x in v)}")
        m.close()
