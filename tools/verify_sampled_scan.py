#!/usr/bin/env python3
"""The cost of speculative sampling (gpt2_decode_verify_sampled) at GPT-2 124M
shapes: V = 50257, page 16, context ~1000, B = 64 and B = 8, 2 / 4 / 8 rows per
sequence.

1. hpa_sample_filtered_prob per launch over R = B x rows dense rows (HIP events
   around LAUNCHES back-to-back launches, five samples: median and max - min),
   with no filter, k = 50, P = 0.9 and both, T = 1; beside it
   hpa_sample_filtered over B rows with the same settings (the same passes plus
   the draw).  Rows are randn * 3.
2. One whole sampled pass (wall clock: the call is host-synchronous) against
   the greedy verify pass of the same rows and against the graph-replayed
   mode-2 decode step, the only route to sampled tokens without it; tokens per
   millisecond at full and at zero acceptance, and the mean number of accepted
   drafts per pass at which the pass breaks even with the step
   (pass / step - 1).  A pass costs the same whatever is accepted.
usage: verify_sampled_scan.py [--steps 200]
HPA_LIB=<path> runs another build of the library."""
import argparse
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

V, P, REPEATS, LAUNCHES = 50257, 16, 5, 10
pa.init(0)
L = pa.lib()
print(f"# {pa.device_info()[0]}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# V = {V}; {LAUNCHES} launches per sample, {REPEATS} samples: median us per launch (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)
D = pa.DeviceBuffer.from_array


def med(v):
    return statistics.median(v), max(v) - min(v)


def sample(fn):
    t.start()
    for _ in range(LAUNCHES):
        fn()
    return t.stop() * 1e3 / LAUNCHES


FILTERS = [("no filter", 0, 1.0), ("k=50", 50, 1.0), ("P=0.9", 0, 0.9), ("k=50 P=0.9", 50, 0.9)]
for B in (64, 8):
    for rows in (2, 4, 8):
        R = B * rows
        x = D((rng.standard_normal((R, V)) * 3).astype(np.float32))
        seq = D((np.arange(R) // rows).astype(np.int32))
        tgt = D(rng.integers(0, V, R).astype(np.int32))
        wt, ws = pa.DeviceBuffer(8 * R), pa.DeviceBuffer(8 * R)
        st = D(np.arange(1, B + 1, dtype=np.uint64))
        nxt = pa.DeviceBuffer(4 * B)
        line = []
        for name, k, p in FILTERS:
            dT, dk, dp = D(np.ones(B, np.float32)), D(np.full(B, k, np.int32)), D(np.full(B, p, np.float32))

            def prob():
                pa.check(L.hpa_sample_filtered_prob(x.ptr, R, V, seq.ptr, dT.ptr, dk.ptr, dp.ptr, tgt.ptr, None, None,
                                                    wt.ptr, ws.ptr), "prob")

            def draw():
                pa.check(L.hpa_sample_filtered(x.ptr, B, V, dT.ptr, dk.ptr, dp.ptr, st.ptr, nxt.ptr, None, None, None,
                                               None, None), "draw")

            for fn in (prob, draw):
                for _ in range(3):
                    fn()
            pa.check(L.hpa_synchronize())
            a, b = [], []
            for _ in range(REPEATS):
                a.append(sample(prob))
                b.append(sample(draw))
            (am, asp), (bm, bsp) = med(a), med(b)
            line.append(f"{name}: prob {am:8.2f} ({asp:5.2f}), {am / R:5.2f} / row; sampler, {B} rows {bm:7.2f} ({bsp:5.2f})")
            for buf in (dT, dk, dp):
                buf.free()
        print(f"B={B:3d} rows={rows} R={R:3d}:  " + "\n" + "\n".join("      " + s for s in line), flush=True)
        for buf in (x, seq, tgt, wt, ws, st, nxt):
            buf.free()

# ---- whole passes against the graph-replayed mode-2 step
MAXC, WIN = 1024, 20
FILL = MAXC - 8 - WIN
print(f"# whole passes: GPT-2 124M, page {P}, ctx ~{FILL}, T = 1 (no filter) unless named; ms per call, median (spread)")
for B in (64, 8):
    m = pa.Model(dict(pa.GPT2_124M), seed=1)
    m.decode_init(B, P, MAXC)
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

    def pass_ms(fn, drafts):
        for _ in range(3):
            m.set_positions(pos)
            fn(drafts)
        total, n = 0.0, 0
        while n < max(10, args.steps // 10):
            m.set_positions(pos)
            t0 = time.perf_counter()
            fn(drafts)
            total += (time.perf_counter() - t0) * 1e3
            n += 1
        return total / n

    greedy = {}
    for rows in (2, 4, 8):
        drafts = [list(range(1, rows))] * B
        greedy[rows] = med([pass_ms(m.verify, drafts) for _ in range(REPEATS)])
    for name, k, p in (("no filter", 0, 1.0), ("k=50 P=0.9", 50, 0.9)):
        m.set_sampling(True, seed=11, filtered=True)
        m.set_sampling_params(-1, temperature=1.0, top_k=k, top_p=p)
        m.set_graph(True)
        sm, ss = med([step_ms() for _ in range(REPEATS)])
        print(f"B={B:3d} {name}: mode-2 decode step (graph, form {m.layer_form()}) {sm:7.4f} ms ({ss:6.4f}) = "
              f"{B / sm:7.1f} tok/ms", flush=True)
        for rows in (2, 4, 8):
            drafts = [list(range(1, rows))] * B
            vm, vs = med([pass_ms(m.verify_sampled, drafts) for _ in range(REPEATS)])
            gm, gs = greedy[rows]
            print(f"      rows={rows}: sampled pass {vm:7.4f} ms ({vs:6.4f})   greedy verify pass {gm:7.4f} ms ({gs:6.4f})   "
                  f"sampled / greedy {vm / gm:4.2f}   {B * rows / vm:7.1f} tok/ms at full acceptance, {B / vm:6.1f} at zero   "
                  f"break-even at {vm / sm - 1:4.2f} accepted of {rows - 1} drafts "
                  f"({'cannot pay off' if vm / sm - 1 > rows - 1 else 'pays off above it'})", flush=True)
        m.set_sampling(False)
    m.close()
