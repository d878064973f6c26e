"""W4A8 in the fused GEMM (hpa_gemm_mx48.hip, w_dtype = HPA_FP4A8): MXFP4 weights x MXFP8 activations.

Pack and quantiser: codes and e8m0 bytes equal the numpy mirrors bit for bit.  GEMM: float64 LayerNorm, the
mirror quantiser, then the float64 product of decode(code) 2^t of both operands; bound SUM_REL sum |a||w| +
2e-6 plus an ambiguous-midpoint term built like gemm_bounds.bf16_operands': an A element within 1e-5
relative of an e4m3 midpoint at its group's scale may round either way under the fp32 LayerNorm, one e4m3
step at its binade times |w|.  A group whose float64 absmax is within 1e-5 relative of a scale-rule
boundary (0.875 2^e, 2^e) would make the scale itself ambiguous under LN: reference() asserts there is
none (without LN the fp32 input is exact).  Groups 2^12 apart in scale in both operands.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_fused import _ln, _stats_tiles
from test_gpu_gemm_fp4w import _check, _weights4

pytestmark = pytest.mark.gpu

# fp32_bound's 4e-6 was set for fp32 MFMA chains; the scaled MFMA's 128-term sum misses it: worst |gpu - ref| /
# sum |a||w| over CASES 5.23e-6 (profiles/r21/w_mx48.txt).  Twice that (runs are bit-deterministic); << 2^-10.
SUM_REL = 2 * 5.23e-6


def _pack(hip, W):
    N, K = W.shape
    codes = hip.DeviceBuffer(hip.lib().hpa_frag_mx4_bytes(N, K))
    scales = hip.DeviceBuffer(hip.lib().hpa_frag_mx4_scale_bytes(N, K))
    hip.check(hip.lib().hpa_pack_frag_mx4(hip.DeviceBuffer.from_array(W).ptr, N, K, K, codes.ptr, scales.ptr), "pack")
    hip.check(hip.lib().hpa_synchronize())
    return codes, scales


@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("K", [128, 160])
def test_pack_equals_mirror(hip, N, K):
    W = _weights4(np.random.default_rng(N + K), N, K)
    W[0, :8] = [0.25, -0.75, 1.25, -1.75, 2.5, -3.5, 5.0, 6.0]  # ties, at t = 0 of a group the 6 leads
    W[0, 8:32] = 0
    codes, scales = _pack(hip, W)
    want_c, want_s, _ = hip.quantize_mxfp4_rows(W)
    Np, Kp = (N + 15) // 16 * 16, (K + 127) // 128 * 128
    assert hip.lib().hpa_frag_mx4_bytes(N, K) == Np * Kp // 2 and hip.lib().hpa_frag_mx4_scale_bytes(N, K) == Np * 16
    got = hip.from_frag_mx4(codes.download(Np * Kp // 2, np.uint8), Np, Kp)
    assert np.array_equal(got[:N, :K], want_c) and not got[N:].any() and not got[:, K:].any()
    assert got[0, :8].tolist() == [0, 8 | 2, 2, 8 | 4, 4, 8 | 6, 6, 7]  # pins the nibble order too
    s = hip.from_frag_mx4_scales(scales.download(Np * 16, np.uint8), Np, 512)  # the whole dword: steps 0..3
    assert np.array_equal(s[:N, :K // 32], want_s) and np.all(s[N:] == 127) and np.all(s[:, K // 32:] == 127)


def _acts(rng, M, K, ln):  # a row is the same at every M; not normalised: even groups scaled by 2^-12
    x = rng.uniform(-1, 1, (max(M, 64), K)).astype(np.float32)[:M]
    if not ln:
        x.reshape(M, K // 32, 32)[:, ::2] *= np.float32(2.0 ** -12)
    return x


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("K", [128, 160])
def test_quantiser_equals_mirror(hip, M, K):
    x = _acts(np.random.default_rng(M + K), M, K, False)
    up = np.nextafter(np.float32(448), np.float32(1e9))
    x[0, :96] = 0  # group 0: absmax 448 with the ties and the subnormal range; 1: the next float; 2: m = 0.875; 3 stays
    x[0, :10] = [448, 17, 19, -17, 1.5 * 2 ** -9, 2.5 * 2 ** -9, 0.5 * 2 ** -9, 0.51 * 2 ** -9, 7.5 * 2 ** -9, -2.0 ** -9]
    x[0, 32:35] = [up, 17, -19]
    x[0, 64:67] = [0.875 * 2 ** -20, 2.0 ** -22, 2.0 ** -40]
    if M > 1:
        x[1, :64] = 0       # a zero group, and a clamped t
        x[1, 32] = 2.0 ** 100
    ws = hip.DeviceBuffer(hip.lib().hpa_mxfp8_workspace_bytes(M, K))
    hip.check(hip.lib().hpa_quant_mxfp8_rows(hip.DeviceBuffer.from_array(hip.to_frag(x)).ptr, M, K, None, 0, None, None, ws.ptr))
    hip.check(hip.lib().hpa_synchronize())
    Mp, Kp = (M + 15) // 16 * 16, (K + 127) // 128 * 128
    assert ws.nbytes == Mp * Kp + Mp * 16
    codes, s = hip.from_mxfp8_workspace(ws.download(ws.nbytes, np.uint8), M, K)
    want_c, want_s, _ = hip.quantize_mxfp8_rows(x)
    assert np.array_equal(codes[:M, :K], want_c) and not codes[M:].any() and not codes[:, K:].any()
    assert np.array_equal(s[:M, :K // 32], want_s) and np.all(s[M:] == 127) and np.all(s[:, K // 32:] == 127)


def reference(hip, x, W, ln=None):
    """(a', W', bound) in float64: mirror-quantised LayerNorm'ed activations, dequantised weights"""
    a = _ln(x.astype(np.float64), *ln) if ln else x.astype(np.float64)
    M, K = a.shape
    if ln:
        m = np.frexp(np.abs(a).reshape(M, K // 32, 32).max(-1))[0]
        assert np.all(np.minimum(np.abs(m - 0.875), np.minimum(m - 0.5, 1 - m)) > 1e-5), "ambiguous group scale: another seed"
    _, sb, ad = hip.quantize_mxfp8_rows(a)
    Wd = hip.quantize_mxfp4_rows(W)[2].astype(np.float64)
    scale = np.exp2(sb.astype(np.float64) - 127).repeat(32, 1)
    y = np.abs(a) / scale
    step = np.exp2(np.maximum(np.floor(np.log2(np.maximum(y, 2.0 ** -9))), -6) - 3)  # e4m3 spacing at y
    amb = np.abs(y / step - np.floor(y / step) - 0.5) * step <= 1e-5 * y
    return ad, Wd, SUM_REL * (np.abs(ad) @ np.abs(Wd).T) + 2e-6 + (amb * step * scale) @ np.abs(Wd).T


def _launch(hip, epi, M, K, N, waves, rb, ct, ln, seed, pool=None, mutate=None):
    """one launch -> (downloads by name, float64 reference with bias, bound); mutate: the status alone"""
    rng = np.random.default_rng(seed)
    x, W = _acts(rng, M, K, ln), _weights4(rng, N, K)
    bias = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    lw, lb = rng.uniform(0.8, 1.2, K).astype(np.float32), rng.uniform(-0.1, 0.1, K).astype(np.float32)
    res = rng.uniform(-1, 1, (max(M, 64), N)).astype(np.float32)[:M]
    Mp, ntn = (M + 15) // 16 * 16, (N + 15) // 16
    keep, out, bt, pos = list(_pack(hip, W)) + [hip.DeviceBuffer(hip.lib().hpa_mxfp8_workspace_bytes(M, K))], {}, None, None

    def dev(a):
        keep.append(hip.DeviceBuffer.from_array(np.ascontiguousarray(a)))
        return keep[-1].ptr

    def buf(name, n):
        out[name] = hip.DeviceBuffer(n * 4)
        return out[name].ptr

    g = hip.HpaFusedGemm()
    g.x, g.M, g.K, g.N, g.w, g.w_gscale, g.a_ws, g.w_dtype = dev(hip.to_frag(x)), M, K, N, keep[0].ptr, keep[1].ptr, keep[2].ptr, hip.HPA_FP4A8
    g.waves, g.row_blocks, g.col_tiles, g.variant, g.epilogue, g.bias = waves, rb, ct, 1, epi, dev(bias)
    if ln:
        g.ln_stats, g.ln_ntiles, g.ln_w, g.ln_b = dev(_stats_tiles(x, Mp)), K // 16, dev(lw), dev(lb)
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
    a, Wd, bound = reference(hip, x, W, (lw, lb) if ln else None)
    out = {k: v.download(v.nbytes // 4) for k, v in out.items()}
    out.update(res=res, bt=bt, pos=pos)
    return out, a @ Wd.T + bias, bound


# epilogue, M, K, N, waves, row blocks, column tiles, LN, seed (the smallest at which reference() holds, found on
# the CPU).  K = 128: one step; 768: 6 steps and 1600 (padded to 1664): 13, neither divisible by the waves.
# Frag-layout outputs need N % 16 == 0, so N = 40 (a partial row block of W) is the pack test's
CASES = [("RESID", 1, 128, 16, 4, 1, 1, False, 1), ("GELU", 17, 768, 48, 4, 2, 1, True, 1), ("QKV", 17, 128, 384, 8, 1, 1, True, 1),
         ("QKV8", 64, 768, 384, 4, 4, 2, True, 1), ("RESID", 64, 1600, 48, 8, 4, 2, True, 4), ("RESID", 17, 1600, 48, 4, 2, 2, False, 1),
         ("GELU", 64, 128, 48, 8, 2, 2, False, 1), ("RESID", 64, 768, 16, 8, 4, 1, True, 1)]


@pytest.mark.parametrize("epi,M,K,N,waves,rb,ct,ln,seed", CASES)
def test_kernel_against_float64(hip, epi, M, K, N, waves, rb, ct, ln, seed):
    e = getattr(hip, "HPA_FEPI_" + epi.rstrip("8"))
    pool = hip.Pool(1, 2, 16, 4 * M, dtype=hip.HPA_FP8 if epi == "QKV8" else hip.HPA_F32) if epi[0] == "Q" else None
    out, ref, bound = _launch(hip, e, M, K, N, waves, rb, ct, ln, seed, pool=pool)
    _check(hip, epi, M, N, out, ref, bound, pool)


@pytest.mark.parametrize("waves", [4, 8])
def test_rows_independent_of_shape(hip, waves):
    """a row depends on the waves only: bit-identical across M, row blocks and column tiles"""
    outs = []
    for M, rb, ct in ((64, 4, 2), (64, 1, 1), (64, 2, 2), (64, 4, 1), (33, 1, 1), (1, 1, 1)):
        out = _launch(hip, hip.HPA_FEPI_RESID, M, 768, 48, waves, rb, ct, True, seed=1)[0]
        outs.append(hip.from_frag(out["frag"], M, 48).view(np.uint32))
    assert all(np.array_equal(o, outs[0][:o.shape[0]]) for o in outs[1:])


@pytest.mark.parametrize("field,value,says", [("w_gscale", None, "w_gscale"), ("a_ws", None, "a_ws"), ("K", 48, "K % 32"),
                                              ("epilogue", "LOGITS", "epilogue"), ("ln_fold_c1", 16, "ln_fold_c1")])
def test_refusals(hip, field, value, says):  # each with its own message and nothing launched
    value = hip.HPA_FEPI_LOGITS if value == "LOGITS" else value
    rc = _launch(hip, hip.HPA_FEPI_GELU, 16, 128, 16, 4, 1, 1, True, seed=1, mutate=lambda g: setattr(g, field, value))
    err = hip.lib().hpa_last_error().decode()
    assert rc != 0 and "W4A8" in err and says in err
