#!/usr/bin/env python3
"""The attention of a speculative verify pass at GPT-2 124M shapes (12 heads,
page 16, the last row's context 1000), B = 64 and B = 8, 2, 4 and 8 query rows
per sequence, fp32 pool.  HIP events around 20 back-to-back launches, five
repeats, the three kernels alternating (median per launch, and the spread
max - min):
  * verify:  hpa_paged_attention_verify (the few-row kernel);
  * prefill: hpa_paged_attention_prefill_ragged on the same inputs -- the only
    route the parent commit has, the baseline;
  * decode:  one hpa_paged_attention_decode launch (one row per sequence,
    single pass, the engine's waves): the floor for reading the same K/V once.
Consecutive launches walk over 64 / B copies of the batch in different pages,
so every launch streams from HBM (one B = 8 batch alone, 49 MB, would sit in
the 256 MB MALL).
Then one whole gpt2_decode_verify pass of 4 rows per sequence (wall clock: the
call is host-synchronous) against the graph-replayed decode step of the same
engine, as tokens per millisecond at full and at zero acceptance.
usage: verify_scan.py [--steps 200]
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

pa.init(0)
L = pa.lib()
ncu = pa.device_info()[1]
print(f"# {pa.device_info()[0]}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# GPT-2 124M heads, page {P}, ctx {CTX}, fp32 pool; {LAUNCHES} launches per sample, {REPEATS} samples: "
      f"median us per launch (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)


def med(v):
    return statistics.median(v), max(v) - min(v)


def fi(buf):
    return ctypes.cast(buf.ptr, _I)


def ff(buf):
    return ctypes.cast(buf.ptr, _F)


for B in (64, 8):
    nsets = max(1, 64 // B)
    npg = (CTX + P - 1) // P
    pool = pa.Pool(1, NH, P, nsets * B * npg)
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

        def verify(i):
            pa.check(L.hpa_paged_attention_verify(ff(d_q), pool.ref, 0, fi(d_bt[i % nsets]), npg, fi(d_start),
                                                  fi(d_row0), fi(d_len), B, rows, ff(d_out)), "verify")

        def prefill(i):
            pa.check(L.hpa_paged_attention_prefill_ragged(ff(d_q), pool.ref, 0, fi(d_bt[i % nsets]), npg, fi(d_start),
                                                          fi(d_row0), fi(d_len), B, rows, ff(d_out)), "prefill")

        def decode(i):
            pa.check(L.hpa_paged_attention_decode_split_w(d_q1.ptr, pool.ref, 0, d_bt[i % nsets].ptr, npg, d_pos.ptr,
                                                          d_o1.ptr, B, 1, None, 1, waves), "decode")

        def sample(fn):
            t.start()
            for i in range(LAUNCHES):
                fn(i)
            return t.stop() * 1e3 / LAUNCHES

        for fn in (verify, prefill, decode):  # warm-up: code objects, clocks
            for i in range(4):
                fn(i)
        pa.check(L.hpa_synchronize())
        v, p, d = [], [], []
        for _ in range(REPEATS):
            v.append(sample(verify))
            p.append(sample(prefill))
            d.append(sample(decode))
        (vm, vs), (pm, ps), (dm, ds) = med(v), med(p), med(d)
        wins = pm - vm > max(vs, ps)
        print(f"B={B:3d} rows={rows}: verify {vm:8.2f} us ({vs:5.2f})   prefill {pm:8.2f} us ({ps:5.2f})   "
              f"decode ({waves} waves, S=1) {dm:7.2f} us ({ds:5.2f})   prefill / verify {pm / vm:5.2f}   "
              f"verify / decode {vm / dm:4.2f}   verify {'wins' if wins else 'does not win'}", flush=True)
        print(f"    repeats verify  {' '.join(f'{x:.2f}' for x in v)}")
        print(f"    repeats prefill {' '.join(f'{x:.2f}' for x in p)}")
        print(f"    repeats decode  {' '.join(f'{x:.2f}' for x in d)}", flush=True)
        for b in (d_q, d_out, d_start, d_row0, d_len):
            b.free()
    for b in d_bt + [d_pos, d_q1, d_o1]:
        b.free()
    del pool

# ---- one whole verify pass of 4 rows against the graph-replayed decode step
ROWS, MAXC, WIN = 4, 1024, 20
FILL = MAXC - 4 - WIN
for B in (64, 8):
    m = pa.Model(dict(pa.GPT2_124M), seed=1)
    m.decode_init(B, P, MAXC)
    m.fill_random(FILL, seed=3)
    m.set_graph(True)
    m.step(np.zeros(B, np.int32))  # a valid pending id per sequence
    pos = np.full(B, FILL, np.int32)
    drafts = [[1, 2, 3]] * B

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

    def pass_ms(request):
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

    st, pv, pp = [], [], []
    for _ in range(REPEATS):
        st.append(step_ms())
        pv.append(pass_ms(0))
        pp.append(pass_ms(1))
    (sm, ss), (vm, vs), (pm, ps) = med(st), med(pv), med(pp)
    print(f"B={B:3d} ctx~{FILL}: decode step (graph, form {m.layer_form()}) {sm:7.4f} ms ({ss:6.4f}) = {B / sm:7.1f} tok/ms   "
          f"verify pass, {ROWS} rows, plan {pa.verify_plan(ROWS, 0, P)}: {vm:7.4f} ms ({vs:6.4f}) = "
          f"{B * ROWS / vm:7.1f} tok/ms at full acceptance, {B / vm:7.1f} at zero   "
          f"with the prefill kernel: {pm:7.4f} ms ({ps:6.4f})", flush=True)
    print(f"    repeats step    {' '.join(f'{x:.4f}' for x in st)}")
    print(f"    repeats verify  {' '.join(f'{x:.4f}' for x in pv)}")
    print(f"    repeats prefill {' '.join(f'{x:.4f}' for x in pp)}", flush=True)
    m.close()
