"""MXFP4 weights in the fused GEMM (hpa_gemm_fp4w.hip, w_dtype = HPA_FP4).

Pack: the device's codes and e8m0 bytes equal the numpy mirror (pagedattn.quantize_mxfp4_rows)
bit for bit.  Kernels (looped, variant 1; A-resident, variant 5): the QKV, RESID and GELU
epilogues against the float64 product of the bf16-rounded A and W' = decode(code) * 2^t.  Bound,
the project's own bars: gemm_bounds.fp32_bound on those operands plus the ambiguous-midpoint term
of gemm_bounds.bf16_operands; the scale is applied at decode, so there is no scale-multiply
term.  Row absmax spans 2^-30 .. 2^10 and neighbouring groups of a row differ by 2^12 in scale,
so a scale taken from the wrong group or row cannot hide.
"""
import ctypes

import numpy as np
import pytest

from gemm_bounds import bf16_operands, fp32_bound
from test_gpu_fused import _gelu_tanh, _ln, _stats_tiles
from test_gpu_gemm_fp8w import CASES, _weights

pytestmark = pytest.mark.gpu


def _weights4(rng, N, K):
    """the fp8 file's rows (absmax 2^-30 .. 2^10, a zero row), odd groups of 32 scaled by 2^12"""
    W = _weights(rng, N, K).reshape(N, K // 32, 32)
    W[:, 1::2] *= np.float32(2.0 ** 12)
    return W.reshape(N, K)


def _pack(hip, W):
    N, K = W.shape
    codes = hip.DeviceBuffer(hip.lib().hpa_frag_fp4_bytes(N, K))
    scales = hip.DeviceBuffer(hip.lib().hpa_frag_mx_scale_bytes(N, K))
    src = hip.DeviceBuffer.from_array(W)
    hip.check(hip.lib().hpa_pack_frag_fp4(src.ptr, N, K, K, codes.ptr, scales.ptr), "pack")
    hip.check(hip.lib().hpa_synchronize())
    return codes, scales


@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("K", [64, 192])
def test_pack_equals_mirror(hip, N, K):
    W = _weights4(np.random.default_rng(N + K), N, K)
    W[1, :8] = [0.25, -0.75, 1.25, -1.75, 2.5, -3.5, 5.0, 6.0]  # ties, at t = 0 of a group the 6 leads
    W[1, 8:32] = 0
    codes, scales = _pack(hip, W)
    want_c, want_s, _ = hip.quantize_mxfp4_rows(W)
    Np = (N + 15) // 16 * 16
    assert hip.lib().hpa_frag_fp4_bytes(N, K) == Np * K // 2 and hip.lib().hpa_frag_mx_scale_bytes(N, K) == Np * K // 32
    got = hip.from_frag_fp4(codes.download(Np * K // 2, np.uint8), Np, K)
    assert np.array_equal(got[:N], want_c) and np.all(got[N:] == 0)  # padded rows: code 0, byte 127
    assert got[1, :8].tolist() == [0, 8 | 2, 2, 8 | 4, 4, 8 | 6, 6, 7]  # pins the nibble order too
    s = hip.from_frag_mx_scales(scales.download(Np * K // 32, np.uint8), Np, K)
    assert np.array_equal(s[:N], want_s) and np.all(s[N:] == 127)


def _launch(hip, epi, M, K, N, waves, rb, ct, ln, seed, variant=1, pool=None, mutate=None):
    """one launch on seeded operands -> (downloads by name, float64 reference with bias, bound);
    with mutate: the descriptor is changed first and only the status comes back"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (max(M, 64), K)).astype(np.float32)[:M]  # a row is the same at every M
    W = _weights4(rng, N, K)
    bias = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    lw, lb = rng.uniform(0.8, 1.2, K).astype(np.float32), rng.uniform(-0.1, 0.1, K).astype(np.float32)
    res = rng.uniform(-1, 1, (max(M, 64), N)).astype(np.float32)[:M]
    Mp, ntn = (M + 15) // 16 * 16, (N + 15) // 16
    keep, out, bt, pos = list(_pack(hip, W)), {}, None, None

    def dev(a):
        keep.append(hip.DeviceBuffer.from_array(np.ascontiguousarray(a)))
        return keep[-1].ptr

    def buf(name, n):
        out[name] = hip.DeviceBuffer(n * 4)
        return out[name].ptr

    g = hip.HpaFusedGemm()
    g.x, g.M, g.K, g.N, g.w, g.w_gscale, g.w_dtype = dev(hip.to_frag(x)), M, K, N, keep[0].ptr, keep[1].ptr, hip.HPA_FP4
    g.waves, g.row_blocks, g.col_tiles, g.variant, g.epilogue, g.bias = waves, rb, ct, variant, epi, dev(bias)
    a = x.astype(np.float64)
    if ln:
        g.ln_stats, g.ln_ntiles, g.ln_w, g.ln_b = dev(_stats_tiles(x, Mp)), K // 16, dev(lw), dev(lb)
        a = _ln(a, lw, lb)
    if epi == hip.HPA_FEPI_RESID:
        g.res_in, g.out, g.stats_out = dev(hip.to_frag(res)), buf("frag", Mp * N), buf("stats", ntn * Mp * 2)
    elif epi == hip.HPA_FEPI_QKV:  # sequence m on pages 4m .. 4m+3, at position 7m % 64
        bt, pos = np.arange(4 * M, dtype=np.int32).reshape(M, 4), (7 * np.arange(M) % 64).astype(np.int32)
        g.out, g.pool, g.block_table, g.bt_stride, g.pos = buf("q", M * N // 3), ctypes.pointer(pool.s), dev(bt), 4, dev(pos)
    else:  # GELU; a refusal case may turn it into LOGITS
        g.out, g.part_out = buf("frag", Mp * N), buf("part", ntn * Mp * 2)
    if mutate:
        mutate(g)
        return hip.lib().hpa_gemm_fused(ctypes.byref(g))
    hip.check(hip.lib().hpa_gemm_fused(ctypes.byref(g)), "gemm_fused")
    hip.check(hip.lib().hpa_synchronize())
    a, Wd, extra = bf16_operands(a, hip.quantize_mxfp4_rows(W)[2])
    out = {k: v.download(v.nbytes // 4) for k, v in out.items()}
    out.update(res=res, bt=bt, pos=pos)
    return out, a @ Wd.T + bias, fp32_bound(a, Wd) + extra


def _check(hip, epi, M, N, out, ref, bound, pool):
    Mp, ntn = (M + 15) // 16 * 16, (N + 15) // 16
    if epi == "RESID":
        got = hip.from_frag(out["frag"], Mp, N)
        assert np.all(np.abs(got[:M] - (out["res"] + ref)) <= bound + 1e-6) and np.all(got[M:] == 0)
        g16 = got[:M].astype(np.float64).reshape(M, ntn, 16)  # stats: the sums of what was stored (test_gpu_fused's bar)
        assert np.all(np.abs(out["stats"].reshape(ntn, Mp, 2)[:, :M, 0].T - g16.sum(-1)) <= 2.0 ** -19 * np.abs(g16).sum(-1))
    elif epi == "GELU":
        assert np.all(np.abs(hip.from_frag(out["frag"], M, N) - _gelu_tanh(ref)) <= 1.2 * bound + 2e-5)  # |gelu'| <= 1.13
    else:
        C = N // 3
        assert np.all(np.abs(out["q"].reshape(M, C) - ref[:, :C]) <= bound[:, :C])
        # an fp8 pool (scale 1) stores e4m3_rne(clamp(value)): half an ulp, 2^-4 relative or 2^-10 below 2^-6
        fmt = (2.0 ** -4 * np.abs(ref) + 2.0 ** -10) if epi == "QKV8" else 0.0
        want = np.clip(ref, -448, 448) if epi == "QKV8" else ref
        for b in range(M):
            k, v = pool.read_tokens(0, out["bt"][b], out["pos"][b] + 1)
            got = np.concatenate([k[out["pos"][b]], v[out["pos"][b]]])
            assert np.all(np.abs(got - want[b, C:]) <= (bound + fmt)[b, C:])


LOOPED = [c for c in CASES if c[0] not in ("LOGITS", "SCORE")] + [("RESID", 17, 1600, 48, 4, 2, 1, True)]  # 25 steps: odd
# A-resident: epilogue, M, K, N, row_blocks, rounds, LN.  N = 48: three column tiles, so a chunk of
# waves * rounds tiles ends mid-round; K = 3200 is past the LayerNorm's width (an fcproj-like GEMM)
ARES = [("RESID", 1, 64, 48, 1, 1, False), ("GELU", 17, 192, 48, 2, 1, True), ("QKV", 64, 768, 384, 4, 2, True),
        ("RESID", 16, 3200, 48, 1, 1, False), ("RESID", 32, 1600, 48, 2, 1, True)]
PICKED = ("GELU", 256, 1600, 6400, 0, 0, 0, True, 0)  # the one shape hpa_fused_pick_fp4 gives the A-resident form, rounds auto


@pytest.mark.parametrize("epi,M,K,N,waves,rb,ct,ln,variant", [c + (1,) for c in LOOPED] + [PICKED] +
                         [(e, M, K, N, w, rb, ct, ln, 5) for e, M, K, N, rb, ct, ln in ARES for w in (4, 8)])
def test_kernel_against_float64(hip, epi, M, K, N, waves, rb, ct, ln, variant):
    e = getattr(hip, "HPA_FEPI_" + epi.rstrip("8"))
    pool = hip.Pool(1, 2, 16, 4 * M, dtype=hip.HPA_FP8 if epi == "QKV8" else hip.HPA_F32) if epi[0] == "Q" else None
    out, ref, bound = _launch(hip, e, M, K, N, waves, rb, ct, ln, seed=M + K + N + waves, variant=variant, pool=pool)
    _check(hip, epi, M, N, out, ref, bound, pool)


def test_pick_follows_the_measured_table(hip):
    """profiles/r20/w_fp4.txt: the A-resident form only for the XL fc from M = 256; looped waves by K alone"""
    def pick(M, N, K):
        out = (ctypes.c_int * 4)()
        hip.lib().hpa_fused_pick_fp4(M, N, K, out)
        return list(out)
    assert pick(256, 6400, 1600) == [5, 4, 2, 0]
    assert [pick(M, N, K)[:2] for M, N, K in ((64, 6400, 1600), (256, 4800, 1600), (256, 3072, 768), (8, 1600, 6400))] == \
        [[1, 4], [1, 4], [1, 4], [1, 8]]


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("variant", [1, 5])
def test_rows_independent_of_shape(hip, waves, variant):
    """looped: a row depends on the waves only, bit-identical across M, row blocks and column tiles;
    A-resident: one in-order k chain, bit-identical across M, row blocks and rounds"""
    outs = []
    for M, rb, ct in ((64, 4, 2), (64, 1, 1), (64, 2, 2), (64, 4, 1), (33, 1, 1), (1, 1, 1)):
        out = _launch(hip, hip.HPA_FEPI_RESID, M, 768, 48, waves, rb, ct, True, seed=3, variant=variant)[0]
        outs.append(hip.from_frag(out["frag"], M, 48).view(np.uint32))
    assert all(np.array_equal(o, outs[0][:o.shape[0]]) for o in outs[1:])


@pytest.mark.parametrize("field,value,variant", [("w_gscale", None, 1), ("K", 96, 1), ("epilogue", "LOGITS", 1),
                                                 ("ln_fold_c1", 16, 1), ("row_blocks", 2, 5)])
def test_refusals(hip, field, value, variant):
    """each refused with a message and nothing launched; the last: variant 5 at row_blocks * K = 2 * 3200"""
    value = hip.HPA_FEPI_LOGITS if value == "LOGITS" else value
    M, K, ln = (32, 3200, False) if variant == 5 else (16, 192, True)
    rc = _launch(hip, hip.HPA_FEPI_GELU, M, K, 16, 4, 1, 1, ln, seed=1, variant=variant, mutate=lambda g: setattr(g, field, value))
    assert rc != 0 and hip.lib().hpa_last_error().decode().strip()
