#!/usr/bin/env python3
"""The fused scoring pass against the only route the parent commit has to the
same numbers, at GPT-2 124M shapes (K = 768, V = 50257), R = 4096 rows in the
engine's default chunks of 1024 rows, fp32 and bf16 weights, HIP events, five
repeats each, the two paths alternating (median, and the spread max - min):
  * SCORE path:  per chunk one SCORE GEMM (HPA_FEPI_SCORE: log-softmax
    epilogue, 16 B of partials per (16-column tile, row), no logits stored)
    and one hpa_score_final;
  * LOGITS path: per chunk the LOGITS GEMM of the same rows, same launch
    shape, into a dense [R][V] fp32 buffer (823 MB) -- what gpt2_forward's
    window path (prefill_all_logits) launches; the log-softmax over that
    buffer would still have to follow, and is not timed.
Then the extra time of the log-probability launch (gpt2_decode_set_logprobs)
in a graph-replayed B = 64 decode step of a synthetic GPT-2 124M, context
~1000, off and on alternating.
usage: score_scan.py [--rows 4096] [--steps 200]
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
ap.add_argument("--rows", type=int, default=4096)
ap.add_argument("--steps", type=int, default=200)
args = ap.parse_args()

K, V, CHUNK, REPEATS = 768, 50257, 1024, 5
R = args.rows
assert R % CHUNK == 0
NT = (V + 15) // 16

pa.init(0)
L = pa.lib()
print(f"# {pa.device_info()[0]}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# K = {K}, V = {V}, R = {R} rows in chunks of {CHUNK}, {REPEATS} repeats: median (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)


def med(v):
    return statistics.median(v), max(v) - min(v)


def stats_tiles(x):
    blk = x.astype(np.float64).reshape(x.shape[0], K // 16, 16)
    st = np.stack([blk.sum(-1), (blk * blk).sum(-1)], -1)  # [rows][tiles][2]
    return np.ascontiguousarray(st.transpose(1, 0, 2), np.float32)


x = rng.uniform(-1, 1, (R, K)).astype(np.float32)
d_x = [pa.DeviceBuffer.from_array(pa.to_frag(x[r:r + CHUNK])) for r in range(0, R, CHUNK)]
d_st = [pa.DeviceBuffer.from_array(stats_tiles(x[r:r + CHUNK])) for r in range(0, R, CHUNK)]
d_lw = pa.DeviceBuffer.from_array(rng.uniform(0.8, 1.2, K).astype(np.float32))
d_lb = pa.DeviceBuffer.from_array(rng.uniform(-0.1, 0.1, K).astype(np.float32))
d_W = pa.DeviceBuffer.from_array(rng.uniform(-0.05, 0.05, (V, K)).astype(np.float32))
d_wf = pa.DeviceBuffer(L.hpa_frag_elems(V, K) * 4)
pa.check(L.hpa_pack_frag(d_W.ptr, V, K, K, d_wf.ptr), "pack")
d_wb = pa.DeviceBuffer(L.hpa_frag_bf16_elems(V, K) * 2)
pa.check(L.hpa_pack_frag_bf16(d_W.ptr, V, K, K, d_wb.ptr), "pack bf16")
d_tgt = pa.DeviceBuffer.from_array(rng.integers(0, V, CHUNK).astype(np.int32))
nf = ctypes.c_size_t()
pa.check(L.hpa_score_workspace(V, CHUNK, ctypes.byref(nf)), "workspace")
d_spart = pa.DeviceBuffer(nf.value * 4)
d_lp, d_top = pa.DeviceBuffer(CHUNK * 4), pa.DeviceBuffer(CHUNK * 4)
d_dense = pa.DeviceBuffer(R * V * 4)
d_part = pa.DeviceBuffer(NT * CHUNK * 2 * 4)
pa.check(L.hpa_synchronize())


def desc(c, bf16, epi):
    g = pa.HpaFusedGemm()
    g.x, g.M, g.K, g.N = d_x[c].ptr, CHUNK, K, V
    g.ln_stats, g.ln_ntiles, g.ln_w, g.ln_b = d_st[c].ptr, K // 16, d_lw.ptr, d_lb.ptr
    g.w, g.w_dtype, g.epilogue = (d_wb.ptr, pa.HPA_BF16, epi) if bf16 else (d_wf.ptr, pa.HPA_F32, epi)
    return g


def score_path(bf16):
    for c in range(R // CHUNK):
        g = desc(c, bf16, pa.HPA_FEPI_SCORE)
        g.score_target, g.score_part = d_tgt.ptr, d_spart.ptr
        pa.check(L.hpa_gemm_fused(ctypes.byref(g)), "SCORE")
        pa.check(L.hpa_score_final(d_spart.ptr, NT, CHUNK, CHUNK, d_lp.ptr, None, d_top.ptr, None), "final")


def logits_path(bf16):
    for c in range(R // CHUNK):
        g = desc(c, bf16, pa.HPA_FEPI_LOGITS)
        g.out, g.part_out = d_dense.ptr + c * CHUNK * V * 4, d_part.ptr
        pa.check(L.hpa_gemm_fused(ctypes.byref(g)), "LOGITS")


def final_only(bf16):
    """the hpa_score_final launches of one SCORE path alone (on the last chunk's partials)"""
    for c in range(R // CHUNK):
        pa.check(L.hpa_score_final(d_spart.ptr, NT, CHUNK, CHUNK, d_lp.ptr, None, d_top.ptr, None), "final")


def timed(fn, bf16):
    t.start()
    fn(bf16)
    return t.stop()


for bf16 in (False, True):
    name = "bf16" if bf16 else "fp32"
    for _ in range(3):  # warm-up: code objects, the dense buffer's pages, the clocks
        for fn in (score_path, logits_path):
            fn(bf16)
    pa.check(L.hpa_synchronize())
    s, lo, fo = [], [], []
    for _ in range(REPEATS):
        s.append(timed(score_path, bf16))
        lo.append(timed(logits_path, bf16))
        fo.append(timed(final_only, bf16))
    (sm, ss), (lm, ls), (fm, fs) = med(s), med(lo), med(fo)
    print(f"{name} weights, R={R}: SCORE path {sm:8.3f} ms (spread {ss:6.3f})   LOGITS path {lm:8.3f} ms "
          f"(spread {ls:6.3f})   SCORE / LOGITS {sm / lm:5.3f}   bytes not written {R * V * 4 / 1e6:.0f} MB", flush=True)
    print(f"    of the SCORE path, the {R // CHUNK} hpa_score_final launches alone: {fm:6.3f} ms (spread {fs:5.3f})")
    print(f"    repeats SCORE  {' '.join(f'{v:.3f}' for v in s)}")
    print(f"    repeats LOGITS {' '.join(f'{v:.3f}' for v in lo)}", flush=True)
for b in (d_dense, d_spart, d_wf, d_wb, d_W):
    b.free()

# ---- the decode step with and without the log-probability launch
B, P, CTX, WIN = 64, 16, 1024, 20
FILL = CTX - 4 - WIN
m = pa.Model(dict(pa.GPT2_124M), seed=1)
m.decode_init(B, P, CTX)
m.fill_random(FILL, seed=3)
m.set_graph(True)
m.step(np.zeros(B, np.int32))
pos = np.full(B, FILL, np.int32)


def step_ms():
    m.set_positions(pos)
    for _ in range(WIN):  # warm-up window: captures the graph of this setting
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


off, on = [], []
for _ in range(REPEATS):
    m.set_logprobs(False)
    off.append(step_ms())
    m.set_logprobs(True)
    on.append(step_ms())
(fm, fs), (nm, ns) = med(off), med(on)
print(f"decode step B={B} ctx~{FILL + WIN} graph, form={m.layer_form()}: logprobs off {fm:7.4f} ms (spread {fs:6.4f})   "
      f"on {nm:7.4f} ms (spread {ns:6.4f})   extra {1e3 * (nm - fm):6.2f} us")
print(f"    repeats off {' '.join(f'{v:.4f}' for v in off)}")
print(f"    repeats on  {' '.join(f'{v:.4f}' for v in on)}")
m.close()
