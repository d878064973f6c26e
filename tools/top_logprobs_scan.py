#!/usr/bin/env python3
"""hpa_top_logprobs alone, inside the decode step and in gpt2_decode_score_top,
at GPT-2 124M shapes (V = 50257), HIP events, five repeats each (median, and
the spread max - min); every shape is warmed first.
  * the kernel alone at B = 64 and B = 8, k = 1 / 5 / 20: ITERS launches
    captured in one graph and replayed per timing (the figure includes the
    boundary between the two launches of a call and between calls).
    Algorithmic bytes: the row read once, 4 B V.  Beside it the two existing
    passes over the same rows, timed the same way in the same run:
    hpa_logprob_rows and hpa_sample_filtered (temperature 0.8, top-k 50).
    --slices S1 S2 ..: the kernel again at those slice counts (k = 20).
  * the graph-replayed decode step of a synthetic GPT-2 124M at B = 64 and
    B = 8, context ~1000: top log-probabilities off (the step as it was), k = 5
    and k = 20, the engines alternating; and the only earlier route to the same
    information: the off step followed by a device-to-host copy of the [B][V]
    logits into pinned memory, every step.
  * gpt2_decode_score_top (k = 5) against gpt2_decode_score on the same R = 4096
    rows (4 sequences of 1024 tokens), fp32 and bf16 weights, with the bytes of
    the dense chunk workspace.
usage: top_logprobs_scan.py [--iters 200] [--steps 200] [--batches 64 8] [--slices ..] [--kernel-only] [--no-score]
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
ap.add_argument("--slices", type=int, nargs="*", default=[])
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--no-score", action="store_true")
args = ap.parse_args()

V, REPEATS, PEAK = 50257, 5, 8.0e12

pa.init(0)
L = pa.lib()
L.hpa_graph_begin.restype = ctypes.c_int
L.hpa_graph_end.restype = ctypes.c_void_p
L.hpa_graph_launch.argtypes = [ctypes.c_void_p]
L.hpa_graph_destroy.argtypes = [ctypes.c_void_p]
L.hpa_host_alloc.restype = ctypes.c_void_p
L.hpa_host_alloc.argtypes = [ctypes.c_size_t]
L.hpa_host_free.argtypes = [ctypes.c_void_p]
ncu = pa.device_info()[1]
print(f"# {pa.device_info()[0]}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# V = {V}, {REPEATS} repeats: median (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)


def med(v):
    return statistics.median(v), max(v) - min(v)


def replayed(fn, iters):
    """us per call of fn: iters calls captured in one graph, replayed REPEATS times"""
    for _ in range(3):
        fn()  # warm-up
    pa.check(L.hpa_synchronize())
    pa.check(L.hpa_graph_begin(), "graph begin")
    for _ in range(iters):
        fn()
    graph = L.hpa_graph_end()
    assert graph, "graph capture failed"
    pa.check(L.hpa_graph_launch(graph), "graph launch")  # warm-up replay
    pa.check(L.hpa_synchronize())
    us = []
    for _ in range(REPEATS):
        t.start()
        pa.check(L.hpa_graph_launch(graph), "graph launch")
        us.append(1e3 * t.stop() / iters)
    L.hpa_graph_destroy(graph)
    return us


def line(name, us, nbytes):
    m_, s_ = med(us)
    print(f"{name}: {m_:7.2f} us per launch (spread {s_:5.2f})   {nbytes / 1e6:6.2f} MB   "
          f"{nbytes / (m_ * 1e-6) / 1e12:5.2f} TB/s = {nbytes / (m_ * 1e-6) / PEAK:5.3f} of 8 TB/s", flush=True)
    print(f"    repeats {' '.join(f'{v:.2f}' for v in us)}")


# ---- the kernel alone
for B in args.batches:
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    buf = pa.DeviceBuffer.from_array
    d_x = buf(x)
    d_ids, d_lps = pa.DeviceBuffer(B * 20 * 4), pa.DeviceBuffer(B * 20 * 4)
    ws_bytes = B * 256 * (12 + 8 * 20)  # any slice count up to 256
    d_ws = pa.DeviceBuffer(ws_bytes)
    d_next, d_lp = buf(rng.integers(0, V, B).astype(np.int32)), pa.DeviceBuffer(B * 4)
    d_st = buf(np.arange(B, dtype=np.uint64) + np.uint64(1337))
    d_t, d_k, d_p = buf(np.full(B, 0.8, np.float32)), buf(np.full(B, 50, np.int32)), buf(np.full(B, 1.0, np.float32))
    nbytes = B * V * 4

    def top(k, slices=0):
        pa.check(L.hpa_top_logprobs_ws(d_x.ptr, B, V, k, None, None, d_ids.ptr, d_lps.ptr, None, None, d_ws.ptr,
                                       ws_bytes, slices), "hpa_top_logprobs_ws")

    auto = L.hpa_top_logprobs_slices(B, V, ncu)
    for k in (1, 5, 20):
        line(f"hpa_top_logprobs    B={B:3d} k={k:2d} slices={auto:3d}", replayed(lambda: top(k), args.iters), nbytes)
    for s in args.slices:
        line(f"hpa_top_logprobs    B={B:3d} k=20 slices={s:3d}", replayed(lambda: top(20, s), args.iters), nbytes)
    line(f"hpa_logprob_rows    B={B:3d}                 ",
         replayed(lambda: pa.check(L.hpa_logprob_rows(d_x.ptr, B, V, d_next.ptr, None, d_lp.ptr)), args.iters), 2 * nbytes)
    line(f"hpa_sample_filtered B={B:3d} T=0.8 top-k 50   ",
         replayed(lambda: pa.check(L.hpa_sample_filtered(d_x.ptr, B, V, d_t.ptr, d_k.ptr, d_p.ptr, d_st.ptr, d_next.ptr,
                                                         None, None, None, None, None)), args.iters), nbytes)
    for d in (d_x, d_ws):
        d.free()
print("# bytes: hpa_top_logprobs and hpa_sample_filtered are charged one read of the rows, hpa_logprob_rows its two")

if args.kernel_only:
    sys.exit(0)

# ---- the decode step: off, k = 5, k = 20, and off + a copy of the logits to the host
P, CTX, WIN, PROMPT = 16, 1024, 20, 980
for B in args.batches:
    prompt = [rng.integers(0, 5000, PROMPT).astype(np.int32) for _ in range(B)]
    engines = {}
    for k in (0, 5, 20):
        m = pa.Model(dict(pa.GPT2_124M), seed=1)
        m.decode_init(B, P, CTX)
        m.set_graph(True)
        m.set_top_logprobs(k)
        m.prefill_ragged(prompt)
        engines[k] = m
    pos = np.full(B, PROMPT, np.int32)
    host = L.hpa_host_alloc(B * V * 4)
    assert host

    def step_ms(m, copy):
        m.set_positions(pos)
        for _ in range(WIN):  # warm-up window: captures the graph of this setting
            m.step_async()
        total, n = 0.0, 0
        while n < args.steps:
            m.set_positions(pos)
            pa.check(L.hpa_synchronize())
            t.start()
            for _ in range(WIN):
                m.step_async()
                if copy:  # the rows a host-side top-k needs, every step (synchronous: the step's feedback waits)
                    pa.check(L.hpa_memcpy(host, m.logits_ptr(), B * V * 4), "logits to host")
            total += t.stop()
            n += WIN
        m.status()
        return total / n

    res = {name: [] for name in ("off", "k=5", "k=20", "off+copy")}
    for _ in range(REPEATS):
        res["off"].append(step_ms(engines[0], False))
        res["k=5"].append(step_ms(engines[5], False))
        res["k=20"].append(step_ms(engines[20], False))
        res["off+copy"].append(step_ms(engines[0], True))
    fm = med(res["off"])[0]
    print(f"decode step B={B} ctx~{PROMPT + WIN} graph, form={engines[0].layer_form()}; [B][V] logits = {B * V * 4 / 1e6:.2f} MB")
    for name, v in res.items():
        m_, s_ = med(v)
        print(f"    {name:9s} {m_:7.4f} ms (spread {s_:6.4f})   extra {1e3 * (m_ - fm):7.2f} us"
              f"    repeats {' '.join(f'{u:.4f}' for u in v)}", flush=True)
    L.hpa_host_free(host)
    for m in engines.values():
        m.close()

if args.no_score:
    sys.exit(0)

# ---- score_top against score, R = 4096
SEQ, NSEQ, K = 1024, 4, 5
seqs = [rng.integers(0, 5000, SEQ).astype(np.int32) for _ in range(NSEQ)]
for name, kw in (("fp32 weights", {}), ("bf16 weights", dict(kv_dtype=pa.HPA_BF16, w_dtype=pa.HPA_BF16))):
    m = pa.Model(dict(pa.GPT2_124M), seed=1)
    m.decode_init(NSEQ, P, CTX, **kw)
    zero = np.zeros(NSEQ, np.int32)
    res = {"score": [], "score_top": []}
    for r in range(REPEATS + 1):  # the first round warms both and allocates their workspaces
        for which in res:
            m.set_positions(zero)
            pa.check(L.hpa_synchronize())
            t.start()
            if which == "score":
                m.score(seqs)
            else:
                m.score_top(seqs, K)
            ms = t.stop()
            if r:
                res[which].append(ms)
    (sm, ss), (tm, ts) = med(res["score"]), med(res["score_top"])
    print(f"R = {SEQ * NSEQ} rows, {name}: score {sm:8.3f} ms (spread {ss:6.3f})   score_top k={K} {tm:8.3f} ms "
          f"(spread {ts:6.3f})   ratio {tm / sm:5.2f}   dense chunk workspace 256 x {V} x 4 = {256 * V * 4 / 1e6:.1f} MB",
          flush=True)
    print(f"    repeats score     {' '.join(f'{v:.3f}' for v in res['score'])}")
    print(f"    repeats score_top {' '.join(f'{v:.3f}' for v in res['score_top'])}")
    m.close()
