"""W4A8 (HPA_FP4A8, hpa_gemm_mx48.hip) against fp4 looped, fp8 and bf16 weights
(profiles/r21/w_mx48.txt, timing part).  HIP events, median of 5 with max - min, the versions
alternating inside one process (the harness of tools/w_fp4_scan.py).

(a) the four layer GEMMs at GPT-2 124M and XL shapes, M = 8, 64, 256 and 1024 (prefill-sized): the
    activation quantiser alone (hpa_quant_mxfp8_rows), the pair (hpa_gemm_fused: quantiser + GEMM,
    library shape) and their difference (the GEMM: it cannot be launched without its quantiser
    through the interface), against the fp4 looped kernel (the XL fc from M = 256: its A-resident
    default), the fp8 kernel and the bf16 default.
(s) the W4A8 pair over the launch shapes (waves, row blocks, column tiles): the table
    hpa_fused_pick_mx48 follows.
(b) the graph-replayed decode step at 124M and XL, B = 8 and 64, context 512.
(c) one XL prefill pass, 4 sequences of 256 tokens.

Usage: python tools/w_mx48_scan.py [out.txt] [a|s|b|c]
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w_fp4_scan as base  # noqa: E402  (its harness: alternate, gemm for fp4 / fp8 / bf16, say)
from w_fp4_scan import INNER, L, alternate, np, pa, say, synth  # noqa: E402

base.lines[0] = base.lines[0].replace("fp4 weights against fp8 and bf16 weights", "W4A8 against fp4, fp8 and bf16 weights")
SHAPES = ((4, 1, 1), (4, 2, 1), (4, 2, 2), (4, 4, 2), (8, 1, 1), (8, 2, 2), (8, 4, 2))


def layer_gemms():
    for model, C in (("124M", 768), ("XL", 1600)):
        for name, N, K, epi in (("qkv", 3 * C, C, pa.HPA_FEPI_GELU), ("attproj", C, C, pa.HPA_FEPI_RESID),
                                ("fc", 4 * C, C, pa.HPA_FEPI_GELU), ("fcproj", C, 4 * C, pa.HPA_FEPI_RESID)):
            for M in (8, 64, 256, 1024):
                yield model, name, M, N, K, epi


def build48(M, K, N, epi, rng, shapes):
    keep = []

    def dev(a):
        keep.append(pa.DeviceBuffer.from_array(np.ascontiguousarray(a)))
        return keep[-1].ptr

    Mp = (M + 15) // 16 * 16
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = pa.DeviceBuffer.from_array(rng.uniform(-0.05, 0.05, (N, K)).astype(np.float32))
    wb, sc = pa.DeviceBuffer(L.hpa_frag_mx4_bytes(N, K)), pa.DeviceBuffer(L.hpa_frag_mx4_scale_bytes(N, K))
    ws = pa.DeviceBuffer(L.hpa_mxfp8_workspace_bytes(M, K))
    pa.check(L.hpa_pack_frag_mx4(W.ptr, N, K, K, wb.ptr, sc.ptr), "pack mx4")
    keep += [wb, sc, ws]
    xs, ln = dev(pa.to_frag(x)), [None, 0, None, None]
    if epi != pa.HPA_FEPI_RESID:  # LN on the qkv / fc operand, none on attproj / fcproj
        st = np.zeros((K // 16, Mp, 2), np.float32)
        blk = x.astype(np.float64).reshape(M, K // 16, 16)
        st[:, :M, 0], st[:, :M, 1] = blk.sum(-1).T, (blk * blk).sum(-1).T
        ln = [dev(st), K // 16, dev(np.ones(K, np.float32)), dev(np.zeros(K, np.float32))]
    bias, out = dev(np.zeros(N, np.float32)), dev(np.zeros(Mp * N, np.float32))
    res, stats = dev(np.zeros(Mp * N, np.float32)), dev(np.zeros((N // 16, Mp, 2), np.float32))
    pa.check(L.hpa_synchronize())
    del W
    fns = {}
    for shape in shapes:
        g = pa.HpaFusedGemm()
        g.x, g.M, g.K, g.N, g.epilogue, g.w_dtype, g.w, g.w_gscale, g.a_ws = xs, M, K, N, epi, pa.HPA_FP4A8, wb.ptr, sc.ptr, ws.ptr
        g.ln_stats, g.ln_ntiles, g.ln_w, g.ln_b = ln
        g.bias, g.out = bias, out
        g.waves, g.row_blocks, g.col_tiles = shape
        g.variant = 1 if shape[0] else 0
        if epi == pa.HPA_FEPI_RESID:
            g.res_in, g.stats_out = res, stats

        def run(g=g):
            for _ in range(INNER):
                pa.check(L.hpa_gemm_fused(ctypes.byref(g)), "gemm_fused")
        run.keep = keep
        fns[shape] = run

    def quant():
        for _ in range(INNER):
            pa.check(L.hpa_quant_mxfp8_rows(xs, M, K, ln[0], ln[1], ln[2], ln[3], ws.ptr), "quant")
    quant.keep = keep
    return fns, quant


def part_a():
    say("(a) GEMMs: us per launch (spread).  qkv is timed with the GELU epilogue (same N, K and LN; no K/V append).  a8 pair:")
    say("    hpa_gemm_fused on HPA_FP4A8 at the library's shape (quantiser + GEMM); a8 gemm = pair - quant (derived)")
    say(f"{'model':5} {'gemm':8} {'M':>4} {'N':>6} {'K':>5} | {'a8 quant':>14} | {'a8 pair':>14} {'a8 gemm':>7} | {'fp4 looped':>14} | "
        f"{'fp8':>14} | {'bf16 default':>14} | a8/f4  a8/f8  a8/b16  loses to")
    rng = np.random.default_rng(0)
    for model, name, M, N, K, epi in layer_gemms():
        fns, quant = build48(M, K, N, epi, rng, [(0, 0, 0)])
        v = {"a8": fns[(0, 0, 0)], "q": quant, "f4": base.gemm(M, K, N, epi, pa.HPA_FP4, 0 if M >= 256 and N >= 6400 and K == 1600 else 1, rng),
             "f8": base.gemm(M, K, N, epi, pa.HPA_FP8, 1, rng), "b16": base.gemm(M, K, N, epi, pa.HPA_BF16, 0, rng)}
        us = {k: (m / INNER, s / INNER) for k, (m, s) in alternate(v).items()}
        cell = lambda k: f"{us[k][0]:7.2f} ({us[k][1]:4.2f})"  # noqa: E731
        lose = [k for k in ("f4", "f8", "b16") if us["a8"][0] > us[k][0]]
        say(f"{model:5} {name:8} {M:4d} {N:6d} {K:5d} | {cell('q')} | {cell('a8')} {us['a8'][0] - us['q'][0]:7.2f} | {cell('f4')} | "
            f"{cell('f8')} | {cell('b16')} | {us['a8'][0] / us['f4'][0]:.3f}  {us['a8'][0] / us['f8'][0]:.3f}  "
            f"{us['a8'][0] / us['b16'][0]:.3f}   {' '.join(lose) or '-'}")
    say()


def part_s():
    say("(s) the W4A8 pair by launch shape (waves, row blocks, column tiles): us per launch; * the fastest, pick = variant 0")
    say(f"{'model':5} {'gemm':8} {'M':>4} | " + " ".join(f"{str(s):>10}" for s in SHAPES) + f" | {'pick':>7}")
    rng = np.random.default_rng(0)
    for model, name, M, N, K, epi in layer_gemms():
        shapes = [s for s in SHAPES if ((M + 15) // 16) % s[1] == 0]
        fns, _ = build48(M, K, N, epi, rng, shapes + [(0, 0, 0)])
        us = {k: m / INNER for k, (m, _) in alternate(fns).items()}
        best = min(shapes, key=lambda s: us[s])
        say(f"{model:5} {name:8} {M:4d} | " + " ".join((f"{us[s]:9.2f}" + ("*" if s == best else " ")) if s in us else f"{'--':>10}"
                                                       for s in SHAPES) + f" | {us[(0, 0, 0)]:7.2f}")
    say()


VERSIONS = (("a8", pa.HPA_FP4A8), ("fp4", pa.HPA_FP4), ("fp8", pa.HPA_FP8), ("bf16 default", pa.HPA_BF16))


def part_b():
    say("(b) graph-replayed decode step, page 16, fp32 pool, context 513 .. 652: ms per step (spread)")
    for model, cfgd in (("124M", pa.GPT2_124M), ("XL", pa.GPT2_XL)):
        params = synth.params(cfgd, seed=1)
        for B in (8, 64):
            ms = {}
            for name, wd in VERSIONS:
                m = pa.Model(cfgd, params=params)
                m.decode_init(B, 16, 704, w_dtype=wd)
                m.set_graph(True)
                m.fill_random(512, seed=3)
                m.step(np.zeros(B, np.int32))
                ms[name] = m

            def stepper(m):
                def run():
                    for _ in range(INNER):
                        m.step(None, want_next=False)
                return run
            r = alternate({k: stepper(m) for k, m in ms.items()})
            say(f"{model:5} B={B:3d} | " + " | ".join(f"{k} {r[k][0] / INNER / 1e3:7.4f} ({r[k][1] / INNER / 1e3:6.4f})" for k in ms))
            for m in ms.values():
                m.close()
    say()


def part_c():
    say("(c) XL prefill pass, 4 sequences x 256 tokens from position 0, page 16, fp32 pool: ms per pass (spread), host call included")
    params = synth.params(pa.GPT2_XL, seed=1)
    toks = [np.random.default_rng(b).integers(0, 50000, 256).astype(np.int32) for b in range(4)]
    ms = {}
    for name, wd in VERSIONS:
        ms[name] = pa.Model(pa.GPT2_XL, params=params)
        ms[name].decode_init(4, 16, 512, w_dtype=wd)

    def passer(m):
        def run():
            m.set_positions(np.zeros(4, np.int32))
            m.prefill_ragged(toks)
        return run
    r = alternate({k: passer(m) for k, m in ms.items()})
    say("XL    | " + " | ".join(f"{k} {r[k][0] / 1e3:7.3f} ({r[k][1] / 1e3:5.3f})" for k in ms))
    for m in ms.values():
        m.close()
    say()


if __name__ == "__main__":
    which = sys.argv[2] if len(sys.argv) > 2 else "asbc"
    for c, part in (("a", part_a), ("s", part_s), ("b", part_b), ("c", part_c)):
        if c in which:
            part()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(base.lines) + "\n")
