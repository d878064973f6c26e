#!/usr/bin/env python3
"""The cost of sampled tree speculation (gpt2_decode_verify_tree_sampled) at
GPT-2 124M shapes: V = 50257, page 16, context ~1000, B = 64 and B = 8.

1. hpa_sample_filtered_prob_multi over NI = B rows with m = 1, 2, 4, 7 ids per
   row, against hpa_sample_filtered_prob over the m x NI duplicated rows (the
   only route to the same masses without it), with no filter, k = 50, P = 0.9
   and both, T = 1.  HIP events around LAUNCHES back-to-back launches, five
   samples, the two versions alternating: median and max - min.  Rows are
   randn * 3.
2. hpa_sample_filtered_exn over B rows with 0, 1 and 7 excluded ids against
   hpa_sample_filtered_ex with one (the ids are the row's largest logits: all
   kept, so every one of them is removed).
3. One whole pass of 8 nodes per sequence (wall clock: the call is
   host-synchronous) for a chain, a star and a two-level tree, against
   gpt2_decode_verify_sampled of 8 rows and gpt2_decode_verify_tree of the same
   tree on the same engine, and against the graph-replayed mode-2 decode step;
   tokens per millisecond at full and at zero acceptance and the mean number of
   accepted drafts per pass at which the pass breaks even with the step.
usage: verify_tree_sampled_scan.py [--steps 200]
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

V, P, REPEATS, LAUNCHES, NT = 50257, 16, 5, 10, pa.VERIFY_MAX_ROWS - 1
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


def alternate(fa, fb):
    for fn in (fa, fb):
        for _ in range(3):
            fn()
    pa.check(L.hpa_synchronize())
    a, b = [], []
    for _ in range(REPEATS):
        a.append(sample(fa))
        b.append(sample(fb))
    return med(a), med(b)


FILTERS = [("no filter", 0, 1.0), ("k=50", 50, 1.0), ("P=0.9", 0, 0.9), ("k=50 P=0.9", 50, 0.9)]
for B in (64, 8):
    NI = B
    xh = (rng.standard_normal((NI, V)) * 3).astype(np.float32)
    x = D(xh)
    seq = D(np.arange(NI, dtype=np.int32))
    for m in (1, 2, 4, 7):
        R = NI * m
        xd = D(np.repeat(xh, m, axis=0))  # row r of the multi kernel = rows r * m .. of the duplicated route
        seqd = D(np.repeat(np.arange(NI, dtype=np.int32), m))
        ids = rng.integers(0, V, (NI, NT)).astype(np.int32)
        tg, nt = D(ids), D(np.full(NI, m, np.int32))
        dst = D((np.arange(NI)[:, None] * m + np.arange(NT)[None, :]).astype(np.int32))
        tgd = D(np.ascontiguousarray(ids[:, :m]).reshape(-1))
        wt, ws = pa.DeviceBuffer(8 * NI * NT), pa.DeviceBuffer(8 * NI * NT)
        line = []
        for name, k, p in FILTERS:
            dT, dk, dp = D(np.ones(B, np.float32)), D(np.full(B, k, np.int32)), D(np.full(B, p, np.float32))

            def multi():
                pa.check(L.hpa_sample_filtered_prob_multi(x.ptr, NI, V, seq.ptr, dT.ptr, dk.ptr, dp.ptr, tg.ptr, nt.ptr,
                                                          dst.ptr, None, None, wt.ptr, ws.ptr), "prob_multi")

            def dup():
                pa.check(L.hpa_sample_filtered_prob(xd.ptr, R, V, seqd.ptr, dT.ptr, dk.ptr, dp.ptr, tgd.ptr, None, None,
                                                    wt.ptr, ws.ptr), "prob")

            (am, asp), (bm, bsp) = alternate(multi, dup)
            line.append(f"{name}: multi, {NI} rows {am:8.2f} ({asp:5.2f})   single-id, {R} rows {bm:8.2f} ({bsp:5.2f})   "
                        f"multi / single {am / bm:4.2f}")
            for buf in (dT, dk, dp):
                buf.free()
        print(f"B={B:3d} NI={NI:3d} m={m}:\n" + "\n".join("      " + s for s in line), flush=True)
        for buf in (xd, seqd, tg, nt, dst, tgd, wt, ws):
            buf.free()

    # ---- the pick with a list
    top = np.argsort(-xh, axis=1)[:, :NT].astype(np.int32)
    ex1, exn = D(np.ascontiguousarray(top[:, 0])), D(np.ascontiguousarray(top))
    st, nxt = D(np.arange(1, B + 1, dtype=np.uint64)), pa.DeviceBuffer(4 * B)
    line = []
    for name, k, p in FILTERS:
        dT, dk, dp = D(np.ones(B, np.float32)), D(np.full(B, k, np.int32)), D(np.full(B, p, np.float32))

        def ex():
            pa.check(L.hpa_sample_filtered_ex(x.ptr, B, V, dT.ptr, dk.ptr, dp.ptr, st.ptr, nxt.ptr, None, None, None,
                                              None, None, ex1.ptr), "ex")

        parts = []
        for n in (0, 1, 7):
            dn = D(np.full(B, n, np.int32))

            def many():
                pa.check(L.hpa_sample_filtered_exn(x.ptr, B, V, dT.ptr, dk.ptr, dp.ptr, st.ptr, nxt.ptr, None, None,
                                                   None, None, None, exn.ptr, dn.ptr), "exn")

            (am, asp), (bm, bsp) = alternate(many, ex)
            parts.append(f"exn {n} ids {am:7.2f} ({asp:5.2f}) / ex {bm:7.2f} ({bsp:5.2f}) = {am / bm:4.2f}")
            dn.free()
        line.append(f"{name}: " + "   ".join(parts))
        for buf in (dT, dk, dp):
            buf.free()
    print(f"B={B:3d} pick over {B} rows:\n" + "\n".join("      " + s for s in line), flush=True)
    for buf in (x, seq, ex1, exn, st, nxt):
        buf.free()

# ---- whole passes against the graph-replayed mode-2 step
MAXC, WIN = 1024, 20
FILL = MAXC - 8 - WIN
SHAPES = [("chain", [0, 1, 2, 3, 4, 5, 6]), ("star", [0] * 7), ("two-level", [0, 0, 1, 1, 1, 2, 2])]
print(f"# whole passes of 8 nodes: GPT-2 124M, page {P}, ctx ~{FILL}, T = 1; ms per call, median (spread)")
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

    ids = list(range(1, 8))
    greedy = {name: med([pass_ms(m.verify_tree, [(ids, par)] * B) for _ in range(REPEATS)]) for name, par in SHAPES}
    for fname, k, p in (("no filter", 0, 1.0), ("k=50 P=0.9", 50, 0.9)):
        m.set_sampling(True, seed=11, filtered=True)
        m.set_sampling_params(-1, temperature=1.0, top_k=k, top_p=p)
        m.set_graph(True)
        sm, ss = med([step_ms() for _ in range(REPEATS)])
        cm, cs = med([pass_ms(m.verify_sampled, [ids] * B) for _ in range(REPEATS)])
        print(f"B={B:3d} {fname}: mode-2 decode step (graph, form {m.layer_form()}) {sm:7.4f} ms ({ss:6.4f}) = "
              f"{B / sm:7.1f} tok/ms;   sampled chain pass, 8 rows {cm:7.4f} ms ({cs:6.4f})", flush=True)
        for name, par in SHAPES:
            d = [0]
            for q in par:
                d.append(d[q] + 1)
            depth = max(d)
            vm, vs = med([pass_ms(m.verify_tree_sampled, [(ids, par)] * B) for _ in range(REPEATS)])
            gm, gs = greedy[name]
            print(f"      {name:9s}: sampled tree pass {vm:7.4f} ms ({vs:6.4f})   / sampled chain {vm / cm:4.2f}   "
                  f"greedy tree pass {gm:7.4f} ms ({gs:6.4f})   / greedy tree {vm / gm:4.2f}   "
                  f"{B * (depth + 1) / vm:7.1f} tok/ms at full acceptance (depth {depth}), {B / vm:6.1f} at zero   "
                  f"break-even at {vm / sm - 1:4.2f} accepted of at most {depth} "
                  f"({'cannot pay off' if vm / sm - 1 > depth else 'pays off above it'})", flush=True)
        m.set_sampling(False)
    m.close()
