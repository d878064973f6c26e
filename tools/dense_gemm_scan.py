#!/usr/bin/env python3
"""The dense passes' GEMMs on fp32 weights: hpa_gemm_fused variant 7 (the
split-operand kernel, hpa_gemm_split.hip: the bf16 matrix pipe) against variant
1 (the looped fp32-MFMA kernel: the default route), on the same operands.  HIP
events around a few back-to-back launches, five samples after a discarded
warm-up, the two kernels alternating in one process: median us per launch and
the spread max - min, every repeat printed.  Each shape also prints the largest
difference between the two outputs relative to the largest output.
  * per GEMM, both at the engine's dense launch shape (waves 8, row blocks 4,
    column tiles 2): qkv (LN on load, the append to an fp32 pool), attproj, fc
    (LN on load), fcproj of GPT-2 124M and XL at M = 64, 256, 1024 and 7904, and
    the head GEMM (LOGITS, LNf on load) at M = 1024; "picked" is variant 7 at
    hpa_fused_pick_split's shape, what the engine launches under request 1;
  * --sweep: variant 7 alone over (waves, row blocks, column tiles) at M = 1024
    (what hpa_fused_pick_split's table follows);
  * whole passes (wall clock: the calls are host-synchronous) under
    gpt2_decode_set_dense_gemm 1 and 0 on one engine, GPT-2 124M fp32 weights
    and pool: prefill_ragged of 8 x 988 tokens under prefill-attention request
    0 and 3, and a score of 4 x 1024 rows.
The operands are random bits of the right ranges uploaded as frag-layout
buffers as they stand (a permutation of random data): the timings do not read
them back by row.
usage: dense_gemm_scan.py [--passes 5] [--kernels-only] [--sweep] [--models 124M,XL]
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
ap.add_argument("--sweep", action="store_true", help="also sweep variant 7's launch shapes at M = 1024")
ap.add_argument("--models", default="124M,XL")
args = ap.parse_args()

REPEATS, P, SEQ = 5, 16, 1024
MODELS = {"124M": pa.GPT2_124M, "XL": pa.GPT2_XL}
ROWS = (64, 256, 1024, 7904)

pa.init(0)
L = pa.lib()
print(f"# {pa.device_info()[0].strip()}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# fp32 weights; {REPEATS} samples after one discarded, the kernels alternating: median us per launch (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)


def med(v):
    return statistics.median(v), max(v) - min(v)


def verdict(a, b):
    """a against b (median, spread): wins only past the larger of the two spreads"""
    gap, s = b[0] - a[0], max(a[1], b[1])
    return "wins" if gap > s else "loses" if -gap > s else "within the spreads"


def rand(n, lo, hi):
    return pa.DeviceBuffer.from_array(rng.uniform(lo, hi, n).astype(np.float32))


class Gemm:
    """one layer / head GEMM of the dense pass on random operands; run(variant, waves, rb, ct)"""

    def __init__(self, which, cfg, M):
        C, NH, V = cfg["C"], cfg["NH"], cfg["V"]
        K, N = {"qkv": (C, 3 * C), "attproj": (C, C), "fc": (C, 4 * C), "fcproj": (4 * C, C), "head": (C, V)}[which]
        Mp, ntn, Np = (M + 15) // 16 * 16, (N + 15) // 16, (N + 15) // 16 * 16
        self.which, self.M, self.K, self.N, self.keep = which, M, K, N, []
        g = self.g = pa.HpaFusedGemm()
        g.M, g.K, g.N, g.w_dtype = M, K, N, pa.HPA_F32
        g.x, g.w = self.dev(rand(Mp * K, -1, 1)), self.dev(rand(Np * K, -0.05, 0.05))
        if which != "head":
            g.bias = self.dev(rand(N, -0.1, 0.1))
        if which in ("qkv", "fc", "head"):  # LN on load: statistics of mean 0, variance 1 in every row
            st = np.zeros((K // 16, Mp, 2), np.float32)
            st[..., 1] = 16
            g.ln_stats, g.ln_ntiles = self.dev(pa.DeviceBuffer.from_array(st)), K // 16
            g.ln_w, g.ln_b = self.dev(rand(K, 0.8, 1.2)), self.dev(rand(K, -0.1, 0.1))
        self.out_floats = Mp * N
        if which == "qkv":  # row m: sequence m // SEQ at position m % SEQ, its own pages
            nseq, npg = (M + SEQ - 1) // SEQ, SEQ // P
            self.pool = pa.Pool(1, NH, P, nseq * npg, dtype=pa.HPA_F32)
            g.epilogue, g.pool, g.layer, g.bt_stride = pa.HPA_FEPI_QKV, ctypes.pointer(self.pool.s), 0, npg
            g.block_table = self.dev(pa.DeviceBuffer.from_array(np.arange(nseq * npg, dtype=np.int32)))
            g.pos = self.dev(pa.DeviceBuffer.from_array((np.arange(M) % SEQ).astype(np.int32)))
            g.row_seq = self.dev(pa.DeviceBuffer.from_array((np.arange(M) // SEQ).astype(np.int32)))
            self.out_floats = M * C
        elif which == "fc":
            g.epilogue = pa.HPA_FEPI_GELU
        elif which == "head":
            g.epilogue, g.part_out, self.out_floats = pa.HPA_FEPI_LOGITS, self.dev(pa.DeviceBuffer(ntn * Mp * 8)), M * N
        else:
            g.epilogue, g.res_in = pa.HPA_FEPI_RESID, self.dev(rand(Mp * N, -1, 1))
            g.stats_out = self.dev(pa.DeviceBuffer(ntn * Mp * 8))
        self.out = {v: pa.DeviceBuffer(self.out_floats * 4) for v in (7, 1)}
        self.launches = max(2, min(20, int(2e11 / (2.0 * M * K * N))))

    def dev(self, b):
        self.keep.append(b)
        return b.ptr

    def run(self, variant, waves=8, rb=4, ct=2):
        g = self.g
        g.variant, g.waves, g.row_blocks, g.col_tiles, g.out = variant, waves, rb, ct, self.out[variant].ptr
        pa.check(L.hpa_gemm_fused(ctypes.byref(g)), f"{self.which} variant {variant}")

    def sample(self, *a):
        t.start()
        for _ in range(self.launches):
            self.run(*a)
        return t.stop() * 1e3 / self.launches

    def free(self):
        for b in self.keep + list(self.out.values()):
            b.free()


def alternate(runs):
    """runs: name -> sampler; REPEATS samples each after one discarded, alternating"""
    got = {k: [] for k in runs}
    for i in range(REPEATS + 1):
        for k, fn in runs.items():
            x = fn()
            if i:
                got[k].append(x)
    return got


for name in args.models.split(","):
    cfg = MODELS[name]
    for which in ("qkv", "attproj", "fc", "fcproj", "head"):
        for M in ((1024,) if which == "head" else ROWS):
            gm = Gemm(which, cfg, M)
            for v in (7, 1):  # warm-up: code objects, clocks
                gm.run(v)
                gm.run(v)
            pa.check(L.hpa_synchronize())
            o = {v: gm.out[v].download(gm.out_floats) for v in (7, 1)}
            diff = float(np.abs(o[7] - o[1]).max() / np.abs(o[1]).max())
            got = alternate({"split": lambda: gm.sample(7), "looped": lambda: gm.sample(1),
                             "picked": lambda: gm.sample(7, 0, 0, 0)})  # picked: hpa_fused_pick_split's shape
            m = {k: med(v) for k, v in got.items()}
            tf = 2.0 * M * gm.K * gm.N / (m["split"][0] * 1e-6) / 1e12
            print(f"{name:4s} {which:7s} M={M:5d} K={gm.K:5d} N={gm.N:6d}: "
                  + "   ".join(f"{k} {v[0]:9.2f} ({v[1]:7.2f})" for k, v in m.items())
                  + f"   looped / split {m['looped'][0] / m['split'][0]:5.2f}   split {verdict(m['split'], m['looped'])}"
                  + f"   looped / picked {m['looped'][0] / m['picked'][0]:5.2f}   picked {verdict(m['picked'], m['looped'])}"
                  + f"   split {tf:6.1f} TFLOP/s of the fp32 product   max |diff| / max |out| {diff:.2e}", flush=True)
            for k, v in got.items():
                print(f"    repeats {k:7s}{' '.join(f'{x:.2f}' for x in v)}")
            if args.sweep and M == 1024 and which != "head":
                shapes = [(w, rb, ct) for w in (4, 8) for rb in (1, 2, 4) for ct in (1, 2, 4) if (w, rb, ct) != (8, 4, 4)]
                sw = {s: med(v) for s, v in alternate({s: (lambda s=s: gm.sample(7, *s)) for s in shapes}).items()}
                for s, v in sorted(sw.items(), key=lambda kv: kv[1][0]):
                    print(f"    sweep waves {s[0]} row blocks {s[1]} column tiles {s[2]}: {v[0]:9.2f} ({v[1]:7.2f})")
            gm.free()

# ---- whole passes on one engine, request 1 against request 0
if not args.kernels_only:
    m = pa.Model(dict(pa.GPT2_124M), seed=1)
    m.decode_init(8, P, 1024, kv_dtype=pa.HPA_F32)
    for label, B, T, attn, call in (("prefill_ragged 8 x 988, prefill attention 0", 8, 988, 0, "prefill_ragged"),
                                    ("prefill_ragged 8 x 988, prefill attention 3", 8, 988, 3, "prefill_ragged"),
                                    ("score 4 x 1024, prefill attention 0", 4, 1024, 0, "score")):
        seqs = [rng.integers(0, 50257, T).astype(np.int32) if b < B else np.zeros(0, np.int32) for b in range(8)]
        zero = np.zeros(8, np.int32)
        m.set_prefill_attention(attn)

        def pass_ms(request):
            m.set_dense_gemm(request)
            total = 0.0
            for i in range(args.passes + 1):  # the first pass of a sample is its warm-up
                m.set_positions(zero)
                t0 = time.perf_counter()
                getattr(m, call)(seqs)
                if i:
                    total += (time.perf_counter() - t0) * 1e3
            return total / args.passes

        got = alternate({1: lambda: pass_ms(1), 0: lambda: pass_ms(0)})
        md = {k: med(v) for k, v in got.items()}
        print(f"124M fp32 {label}: " + "   ".join(f"request {k}: {v[0]:8.3f} ms ({v[1]:6.3f})" for k, v in md.items())
              + f"   request 0 / request 1 {md[0][0] / md[1][0]:5.2f}   request 1 {verdict(md[1], md[0])}", flush=True)
        for k, v in got.items():
            print(f"    repeats request {k}  {' '.join(f'{x:.3f}' for x in v)}")
    m.set_dense_gemm(0)
    m.close()
