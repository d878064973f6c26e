"""MXFP4 weights against fp8 and bf16 weights (profiles/r20/w_fp4.txt).  HIP events, median
of 5 with max - min, the versions alternating inside one process.

(a) the four layer GEMMs at GPT-2 124M and XL shapes, M = 8, 64, 256: hpa_gemm_fused on fp4
    weights, looped (variant 1) and A-resident (variant 5, where row_blocks * K <= 3200 allows:
    not fcproj), against the fp8-weight kernel and the bf16 library default (variant 0).  20
    launches per timing; weight bytes per second = N * K * 17 / 32 / time for fp4.
(b) the graph-replayed decode step at 124M and XL, B = 8 and 64, context 512: fp4 weights
    against fp8 weights and the bf16 default pick.

Usage: python tools/w_fp4_scan.py [out.txt] [a|b]
"""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm.c-paged_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import pagedattn as pa  # noqa: E402
import synth  # noqa: E402

pa.init(0)
L = pa.lib()
REPS, INNER = 5, 20
_dev = pa.device_info()
lines = [f"fp4 weights against fp8 and bf16 weights, device '{_dev[0].strip()}', {_dev[1]} CUs",
         f"HIP events; median of {REPS} (max - min); versions alternate in one process", ""]


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def stats(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[-1] - xs[0]


def alternate(variants, warm=2):
    got = {k: [] for k in variants}
    t = pa.Timer()
    for r in range(warm + REPS):
        for k, fn in variants.items():
            pa.check(L.hpa_synchronize())
            t.start()
            fn()
            pa.check(L.hpa_event_record(t.b), "event_record")
            pa.check(L.hpa_synchronize())
            ms = L.hpa_event_elapsed_ms(t.a, t.b)
            if r >= warm:
                got[k].append(ms * 1e3)
    return {k: stats(v) for k, v in got.items()}


def gemm(M, K, N, epi, w_dtype, variant, rng):
    keep = []

    def dev(a):
        keep.append(pa.DeviceBuffer.from_array(np.ascontiguousarray(a)))
        return keep[-1].ptr

    Mp = (M + 15) // 16 * 16
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = pa.DeviceBuffer.from_array(rng.uniform(-0.05, 0.05, (N, K)).astype(np.float32))
    g = pa.HpaFusedGemm()
    g.x, g.M, g.K, g.N, g.epilogue, g.variant, g.w_dtype = dev(pa.to_frag(x)), M, K, N, epi, variant, w_dtype
    if w_dtype == pa.HPA_FP4:
        wb = pa.DeviceBuffer(L.hpa_frag_fp4_bytes(N, K))
        sc = pa.DeviceBuffer(L.hpa_frag_mx_scale_bytes(N, K))
        pa.check(L.hpa_pack_frag_fp4(W.ptr, N, K, K, wb.ptr, sc.ptr), "pack fp4")
        g.w_gscale = sc.ptr
        keep.append(sc)
    elif w_dtype == pa.HPA_FP8:
        wb = pa.DeviceBuffer(L.hpa_frag_fp8_bytes(N, K))
        sc = pa.DeviceBuffer((N + 15) // 16 * 16 * 4)
        pa.check(L.hpa_pack_frag_fp8(W.ptr, N, K, K, wb.ptr, sc.ptr), "pack fp8")
        g.w_scale = sc.ptr
        keep.append(sc)
    else:
        wb = pa.DeviceBuffer(L.hpa_frag_bf16_elems(N, K) * 2)
        pa.check(L.hpa_pack_frag_bf16(W.ptr, N, K, K, wb.ptr), "pack bf16")
    keep.append(wb)
    g.w = wb.ptr
    if epi != pa.HPA_FEPI_RESID:  # LN on the qkv / fc operand, none on attproj / fcproj
        st = np.zeros((K // 16, Mp, 2), np.float32)
        blk = x.astype(np.float64).reshape(M, K // 16, 16)
        st[:, :M, 0], st[:, :M, 1] = blk.sum(-1).T, (blk * blk).sum(-1).T
        g.ln_stats, g.ln_ntiles = dev(st), K // 16
        g.ln_w, g.ln_b = dev(np.ones(K, np.float32)), dev(np.zeros(K, np.float32))
    g.bias, g.out = dev(np.zeros(N, np.float32)), dev(np.zeros(Mp * N, np.float32))
    if epi == pa.HPA_FEPI_RESID:
        g.res_in = dev(np.zeros(Mp * N, np.float32))
        g.stats_out = dev(np.zeros((N // 16, Mp, 2), np.float32))
    pa.check(L.hpa_synchronize())
    del W

    def run():
        for _ in range(INNER):
            pa.check(L.hpa_gemm_fused(ctypes.byref(g)), "gemm_fused")
    run.keep = keep
    return run


def part_a():
    say("(a) GEMMs: us per launch (spread); weight GB/s.  qkv is timed with the GELU epilogue (same N, K and LN; no")
    say("    K/V append into a pool).  ares: the A-resident form; -- where row_blocks * K <= 3200 rules it out")
    say(f"{'model':5} {'gemm':8} {'M':>4} {'N':>6} {'K':>5} | {'fp4 looped':>16} {'GB/s':>6} | {'fp4 ares':>16} {'GB/s':>6} | "
        f"{'fp8':>16} {'GB/s':>6} | {'bf16 default':>16} | f4/f8  ares/looped")
    rng = np.random.default_rng(0)
    for model, C in (("124M", 768), ("XL", 1600)):
        shapes = [("qkv", 3 * C, C, pa.HPA_FEPI_GELU), ("attproj", C, C, pa.HPA_FEPI_RESID),
                  ("fc", 4 * C, C, pa.HPA_FEPI_GELU), ("fcproj", C, 4 * C, pa.HPA_FEPI_RESID)]
        for name, N, K, epi in shapes:
            for M in (8, 64, 256):
                v = {"f4": gemm(M, K, N, epi, pa.HPA_FP4, 1, rng), "f8": gemm(M, K, N, epi, pa.HPA_FP8, 1, rng),
                     "b16d": gemm(M, K, N, epi, pa.HPA_BF16, 0, rng)}
                if K <= 3200:
                    v["f4a"] = gemm(M, K, N, epi, pa.HPA_FP4, 5, rng)
                r = alternate(v)
                us = {k: (m / INNER, s / INNER) for k, (m, s) in r.items()}
                f4b = N * K * 17 / 32

                def cell(k, nbytes=None):
                    if k not in us:
                        return f"{'--':>16}" + (f" {'':6}" if nbytes else "")
                    return f"{us[k][0]:8.2f} ({us[k][1]:5.2f})" + (f" {nbytes / us[k][0] / 1e3:6.0f}" if nbytes else "")
                say(f"{model:5} {name:8} {M:4d} {N:6d} {K:5d} | {cell('f4', f4b)} | {cell('f4a', f4b)} | {cell('f8', N * K)} | "
                    f"{cell('b16d')} | {us['f4'][0] / us['f8'][0]:.3f}  " + (f"{us['f4a'][0] / us['f4'][0]:.3f}" if "f4a" in us else "--"))
    say()


def part_b():
    say("(b) graph-replayed decode step, page 16, fp32 pool: ms per step (spread); weight GB/s of the fp4 step")
    say("    context 513 at the first timing, 20 positions more after each: every version runs its r-th timing at the")
    say("    same context, and the seven timings of a version span 513 .. 652")
    for model, cfgd in (("124M", pa.GPT2_124M), ("XL", pa.GPT2_XL)):
        params = synth.params(cfgd, seed=1)
        for B in (8, 64):
            ms = {}
            for name, wd in (("fp4", pa.HPA_FP4), ("fp8", pa.HPA_FP8), ("bf16 default", pa.HPA_BF16)):
                m = pa.Model(cfgd, params=params)
                m.decode_init(B, 16, 704, w_dtype=wd)
                m.set_graph(True)
                m.fill_random(512, seed=3)
                m.step(np.zeros(B, np.int32))
                ms[name] = (m, m.layer_form())

            def stepper(m):  # every version advances alike: 512 + 7 x 20 positions by the end
                def run():
                    for _ in range(INNER):
                        m.step(None, want_next=False)
                return run
            r = alternate({k: stepper(m) for k, (m, _) in ms.items()})
            wbytes = cfgd["L"] * 12 * cfgd["C"] ** 2 * 17 / 32 + cfgd["V"] * cfgd["C"]
            say(f"{model:5} B={B:3d} | " + " | ".join(f"{k} (form {ms[k][1]}) {r[k][0] / INNER / 1e3:7.4f} ({r[k][1] / INNER / 1e3:6.4f})"
                                                      for k in ms) + f" | fp4 weights {wbytes / (r['fp4'][0] / INNER) / 1e3:6.0f} GB/s")
            for m, _ in ms.values():
                m.close()
    say()


if __name__ == "__main__":
    which = sys.argv[2] if len(sys.argv) > 2 else "ab"
    if "a" in which:
        part_a()
    if "b" in which:
        part_b()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
