#!/usr/bin/env python3
"""The logit-processor kernel alone and inside the decode step, at GPT-2 124M
shapes (V = 50257), HIP events, five repeats each (median, and the spread
max - min):
  * hpa_logits_process alone at B = 64 and B = 8, ITERS launches captured in
    one graph and replayed per timing (eager launches from Python arrive more
    slowly than the kernel runs; the figure includes the boundary between two
    dependent launches), in two forms: mode 0 (partials only, no processed rows
    stored) and with the store.  Algorithmic bytes per element: 4 (logit) + 2
    (count), + 4 with the store; reported as bytes per launch and as a fraction
    of 8 TB/s.  Settings: repetition 1.1, presence 0.2, frequency 0.1, 16 bias
    entries per row, counts of ~700 distinct tokens per row.
  * the graph-replayed decode step of a synthetic GPT-2 124M at B = 64 and
    B = 8, context ~1000 (a real prefill of 980 tokens per sequence: the counts
    are populated), processors on (the same settings) against the same step with
    them off, the two engines alternating.
usage: process_scan.py [--iters 200] [--steps 200] [--kernel-only] [--eager]
  --kernel-only --eager: the kernel part alone with plain launches, for a
  profiler's kernel trace (tools/kstats.py reads it)
HPA_LIB=<path> runs another build of the library."""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm.c-paged_amd"))
import numpy as np  # noqa: E402
import pagedattn as pa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--batches", type=int, nargs="+", default=[64, 8])
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--eager", action="store_true")
args = ap.parse_args()

V, REPEATS, NBIAS, PEAK = 50257, 5, 16, 8.0e12
SET = dict(repetition=1.1, presence=0.2, frequency=0.1)

pa.init(0)
L = pa.lib()
L.hpa_graph_begin.restype = ctypes.c_int
L.hpa_graph_end.restype = ctypes.c_void_p
L.hpa_graph_launch.argtypes = [ctypes.c_void_p]
L.hpa_graph_destroy.argtypes = [ctypes.c_void_p]
ncu = pa.device_info()[1]
print(f"# {pa.device_info()[0]}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# V = {V}, {REPEATS} repeats: median (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)


def med(v):
    return statistics.median(v), max(v) - min(v)


# ---- the kernel alone
for B in args.batches:
    Mp = (B + 15) // 16 * 16
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    counts = np.zeros((B, V), np.uint16)
    for b in range(B):
        counts[b, rng.integers(0, V, 700)] = rng.integers(1, 6, 700)
    ids = np.zeros((B, 300), np.int32)
    vals = np.zeros((B, 300), np.float32)
    for b in range(B):
        ids[b, :NBIAS] = rng.permutation(V)[:NBIAS]
        vals[b, :NBIAS] = -np.inf
    buf = pa.DeviceBuffer.from_array
    d_x, d_c = buf(x), buf(counts)
    d_r, d_p, d_f = (buf(np.full(B, SET[k], np.float32)) for k in ("repetition", "presence", "frequency"))
    d_ids, d_vals, d_n = buf(ids), buf(vals), buf(np.full(B, NBIAS, np.int32))
    slices = L.hpa_logits_process_slices(B, V, ncu)
    d_out = pa.DeviceBuffer(B * V * 4)
    d_part = pa.DeviceBuffer(slices * Mp * 8)

    def launches(store):
        for _ in range(args.iters):
            pa.check(L.hpa_logits_process(d_x.ptr, B, V, d_c.ptr, d_r.ptr, d_p.ptr, d_f.ptr, d_ids.ptr, d_vals.ptr,
                                          d_n.ptr, None, d_out.ptr if store else None, d_part.ptr, Mp, slices),
                     "hpa_logits_process")

    for store in (False, True):
        launches(store)  # warm-up
        pa.check(L.hpa_synchronize())
        graph = None
        if not args.eager:
            pa.check(L.hpa_graph_begin(), "graph begin")
            launches(store)
            graph = L.hpa_graph_end()
            assert graph, "graph capture failed"
            pa.check(L.hpa_graph_launch(graph), "graph launch")  # warm-up replay
            pa.check(L.hpa_synchronize())
        us = []
        for _ in range(REPEATS):
            t.start()
            if graph:
                pa.check(L.hpa_graph_launch(graph), "graph launch")
            else:
                launches(store)
            us.append(1e3 * t.stop() / args.iters)
        if graph:
            L.hpa_graph_destroy(graph)
        m_, s_ = med(us)
        nbytes = B * V * (6 + (4 if store else 0))
        print(f"hpa_logits_process B={B:3d} slices={slices:3d} {'with store' if store else 'mode 0    '}: "
              f"{m_:7.2f} us per launch (spread {s_:5.2f})   {nbytes / 1e6:6.2f} MB per launch   "
              f"{nbytes / (m_ * 1e-6) / 1e12:5.2f} TB/s = {nbytes / (m_ * 1e-6) / PEAK:5.3f} of 8 TB/s", flush=True)
        print(f"    repeats {' '.join(f'{v:.2f}' for v in us)}")
    for d in (d_x, d_c, d_out, d_part):
        d.free()

if args.kernel_only:
    sys.exit(0)

# ---- the decode step with processors on and off
P, CTX, WIN, PROMPT = 16, 1024, 20, 980
for B in args.batches:
    engines = {}
    prompt = [rng.integers(0, 5000, PROMPT).astype(np.int32) for _ in range(B)]
    for on in (False, True):
        m = pa.Model(dict(pa.GPT2_124M), seed=1)
        m.decode_init(B, P, CTX)
        m.set_graph(True)
        if on:
            m.set_processors(True)
            m.set_penalties(-1, **SET)
            m.set_logit_bias(-1, np.arange(100, 100 + NBIAS), np.full(NBIAS, -np.inf))
        m.prefill_ragged(prompt)
        engines[on] = m
    pos = np.full(B, PROMPT, np.int32)

    def step_ms(m):
        m.set_positions(pos)
        for _ in range(WIN):  # warm-up window: captures the graph of this setting
            m.step_async()
        total, n = 0.0, 0
        while n < args.steps:
            m.set_positions(pos)  # with processors on: a recount per sequence, outside the timed window
            pa.check(L.hpa_synchronize())
            t.start()
            for _ in range(WIN):
                m.step_async()
            total += t.stop()
            n += WIN
        m.status()
        return total / n

    off, onv = [], []
    for _ in range(REPEATS):
        off.append(step_ms(engines[False]))
        onv.append(step_ms(engines[True]))
    (fm, fs), (nm, ns) = med(off), med(onv)
    print(f"decode step B={B} ctx~{PROMPT + WIN} graph, form={engines[True].layer_form()}: processors off {fm:7.4f} ms "
          f"(spread {fs:6.4f})   on {nm:7.4f} ms (spread {ns:6.4f})   extra {1e3 * (nm - fm):6.2f} us", flush=True)
    print(f"    repeats off {' '.join(f'{v:.4f}' for v in off)}")
    print(f"    repeats on  {' '.join(f'{v:.4f}' for v in onv)}")
    for m in engines.values():
        m.close()
