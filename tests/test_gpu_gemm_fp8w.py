"""fp8 (e4m3fn) weights in the fused GEMM (hpa_gemm_fp8w.hip, w_dtype = HPA_FP8).

Pack: the device's codes and scales equal the numpy mirror (pagedattn.quantize_fp8_rows)
exactly.  Kernel: every epilogue against the float64 product of the bf16-rounded A and
W' = decode(code) * scale.  Bound, the project's own bars: gemm_bounds.fp32_bound on those
operands, the ambiguous-midpoint term of gemm_bounds.bf16_operands, and 2^-23 |ref| for the
one rounding of the scale multiply.  Every case's rows span scales over 2^12 and more, so
a scale applied to the wrong column cannot hide.
"""
import ctypes

import numpy as np
import pytest

from gemm_bounds import bf16_operands, fp32_bound
from test_gpu_fused import _gelu_tanh, _ln, _stats_tiles

pytestmark = pytest.mark.gpu


def _weights(rng, N, K):
    """rows with absmax from 2^-30 to 2^10: among them a zero row, a row whose absmax is
    exactly 448 * 2^e and a row with elements below scale * 2^-6 (e4m3 subnormals)"""
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    ex = rng.integers(-8, 5, N)
    ex[:8] = [-30, 10, -3, 0, 2, -12, 4, -8]
    W *= np.exp2(ex)[:, None].astype(np.float32)
    W[2] = 0
    W[3] *= 0.5
    W[3, 5] = 448 * 2.0 ** -4
    W[4, 1::2] *= 2.0 ** -9
    return W


def _pack(hip, W):
    N, K = W.shape
    codes = hip.DeviceBuffer(hip.lib().hpa_frag_fp8_bytes(N, K))
    scale = hip.DeviceBuffer((N + 15) // 16 * 16 * 4)
    src = hip.DeviceBuffer.from_array(W)
    hip.check(hip.lib().hpa_pack_frag_fp8(src.ptr, N, K, K, codes.ptr, scale.ptr), "pack")
    hip.check(hip.lib().hpa_synchronize())
    return codes, scale


@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("K", [64, 192])
def test_pack_equals_mirror(hip, N, K):
    W = _weights(np.random.default_rng(N + K), N, K)
    codes, scale = _pack(hip, W)
    want_c, want_s, _ = hip.quantize_fp8_rows(W)
    Np = (N + 15) // 16 * 16
    assert hip.lib().hpa_frag_fp8_bytes(N, K) == Np * K
    got = hip.from_frag_fp8(codes.download(Np * K, np.uint8), Np, K)
    assert np.array_equal(got[:N], want_c) and np.all(got[N:] == 0)  # padded rows: code 0, scale 1
    s = scale.download(Np)
    assert np.array_equal(s[:N], want_s) and np.all(s[N:] == 1)


def _launch(hip, epi, M, K, N, waves, rb, ct, ln, seed, pool=None, mutate=None):
    """one launch on seeded operands -> (downloads by name, float64 reference with bias, bound);
    with mutate: the descriptor is changed first and only the status comes back"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (max(M, 64), K)).astype(np.float32)[:M]  # a row is the same at every M
    W = _weights(rng, N, K)
    bias = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    lw, lb = rng.uniform(0.8, 1.2, K).astype(np.float32), rng.uniform(-0.1, 0.1, K).astype(np.float32)
    res = rng.uniform(-1, 1, (max(M, 64), N)).astype(np.float32)[:M]
    Mp, ntn = (M + 15) // 16 * 16, (N + 15) // 16
    keep, out, tgt, bt, pos = list(_pack(hip, W)), {}, None, None, None

    def dev(a):
        keep.append(hip.DeviceBuffer.from_array(np.ascontiguousarray(a)))
        return keep[-1].ptr

    def buf(name, n):
        out[name] = hip.DeviceBuffer(n * 4)
        return out[name].ptr

    g = hip.HpaFusedGemm()
    g.x, g.M, g.K, g.N, g.w, g.w_scale, g.w_dtype = dev(hip.to_frag(x)), M, K, N, keep[0].ptr, keep[1].ptr, hip.HPA_FP8
    g.waves, g.row_blocks, g.col_tiles, g.variant, g.epilogue = waves, rb, ct, 1, epi
    a = x.astype(np.float64)
    if ln:
        g.ln_stats, g.ln_ntiles, g.ln_w, g.ln_b = dev(_stats_tiles(x, Mp)), K // 16, dev(lw), dev(lb)
        a = _ln(a, lw, lb)
    bare = epi in (hip.HPA_FEPI_LOGITS, hip.HPA_FEPI_SCORE)
    if not bare:
        g.bias = dev(bias)
    if epi == hip.HPA_FEPI_RESID:
        g.res_in, g.out, g.stats_out = dev(hip.to_frag(res)), buf("frag", Mp * N), buf("stats", ntn * Mp * 2)
    elif epi == hip.HPA_FEPI_GELU:
        g.out = buf("frag", Mp * N)
    elif epi == hip.HPA_FEPI_LOGITS:
        g.out, g.part_out = buf("rows", M * N), buf("part", ntn * Mp * 2)
    elif epi == hip.HPA_FEPI_SCORE:
        tgt = rng.integers(0, N, M).astype(np.int32)
        g.score_target, g.score_part = dev(tgt), buf("score", ntn * Mp * 4)
    else:  # QKV: sequence m on pages 4m .. 4m+3, at position 7m % 64
        bt, pos = np.arange(4 * M, dtype=np.int32).reshape(M, 4), (7 * np.arange(M) % 64).astype(np.int32)
        g.out, g.pool, g.block_table, g.bt_stride, g.pos = buf("q", M * N // 3), ctypes.pointer(pool.s), dev(bt), 4, dev(pos)
    if mutate:
        mutate(g)
        return hip.lib().hpa_gemm_fused(ctypes.byref(g))
    hip.check(hip.lib().hpa_gemm_fused(ctypes.byref(g)), "gemm_fused")
    hip.check(hip.lib().hpa_synchronize())
    a, Wd, extra = bf16_operands(a, hip.quantize_fp8_rows(W)[2])
    acc = a @ Wd.T
    bound = fp32_bound(a, Wd) + extra + 2.0 ** -23 * np.abs(acc)
    out = {k: v.download(v.nbytes // 4) for k, v in out.items()}
    out.update(res=res, tgt=tgt, bt=bt, pos=pos)
    return out, acc if bare else acc + bias, bound


CASES = [  # epilogue, M, K, N, waves, row_blocks, col_tiles, LN -> the (row_blocks, col_tiles) instance run
    ("RESID", 1, 64, 16, 4, 1, 1, False),    # one fragment: waves 1..3 fold zeros
    ("RESID", 17, 192, 48, 4, 2, 1, True),   # (2, 1); three steps over four waves
    ("RESID", 64, 768, 48, 8, 4, 2, True),   # (4, 2); 12 steps over 8 waves: 6 x 2, two idle; 3 tiles by 2: one past the end
    ("RESID", 64, 768, 48, 4, 4, 1, False),  # (4, 1)
    ("RESID", 80, 768, 48, 4, 1, 1, True),   # five row groups
    ("GELU", 17, 192, 48, 8, 2, 2, True),    # (2, 2)
    ("GELU", 64, 64, 16, 8, 4, 1, False),    # (4, 1); one step, seven waves idle
    ("LOGITS", 17, 768, 40, 4, 2, 2, True),  # N = 40: a tail tile of 8 columns (row-major outputs only)
    ("LOGITS", 64, 192, 40, 4, 4, 2, True),  # (4, 2) at 4 waves
    ("SCORE", 17, 192, 40, 4, 1, 1, True),
    ("SCORE", 80, 768, 40, 8, 1, 1, True),
    ("QKV", 17, 192, 384, 4, 2, 2, True),    # 3C of two heads, fp32 pool
    ("QKV8", 64, 64, 384, 8, 4, 1, True),    # ... fp8 pool
]


@pytest.mark.parametrize("epi,M,K,N,waves,rb,ct,ln", CASES)
def test_kernel_against_float64(hip, epi, M, K, N, waves, rb, ct, ln):
    e = getattr(hip, "HPA_FEPI_" + epi.rstrip("8"))
    pool = hip.Pool(1, 2, 16, 4 * M, dtype=hip.HPA_FP8 if epi == "QKV8" else hip.HPA_F32) if epi[0] == "Q" else None
    out, ref, bound = _launch(hip, e, M, K, N, waves, rb, ct, ln, seed=M + K + N + waves, pool=pool)
    Mp, ntn = (M + 15) // 16 * 16, (N + 15) // 16
    if epi == "RESID":
        got = hip.from_frag(out["frag"], Mp, N)
        assert np.all(np.abs(got[:M] - (out["res"] + ref)) <= bound + 1e-6) and np.all(got[M:] == 0)
        g16 = got[:M].astype(np.float64).reshape(M, ntn, 16)  # stats: the sums of what was stored (test_gpu_fused's bar)
        assert np.all(np.abs(out["stats"].reshape(ntn, Mp, 2)[:, :M, 0].T - g16.sum(-1)) <= 2.0 ** -19 * np.abs(g16).sum(-1))
    elif epi == "GELU":
        assert np.all(np.abs(hip.from_frag(out["frag"], M, N) - _gelu_tanh(ref)) <= 1.2 * bound + 2e-5)  # |gelu'| <= 1.13
    elif epi == "LOGITS":
        got = out["rows"].reshape(M, N)
        assert np.all(np.abs(got - ref) <= bound)
        nxt, part = hip.DeviceBuffer(M * 4), hip.DeviceBuffer.from_array(out["part"])
        hip.check(hip.lib().hpa_argmax_final(part.ptr, ntn, Mp, M, nxt.ptr, None, None, None))
        assert np.array_equal(nxt.download(M, np.int32), got.argmax(-1))
    elif epi == "SCORE":
        part = out["score"].reshape(ntn, Mp, 4)
        for t in range(ntn):
            r, b = ref[:, 16 * t:16 * t + 16], bound[:, 16 * t:16 * t + 16].max(1)
            mx, tc = r.max(1), out["tgt"] - 16 * t
            assert np.all(np.abs(part[t, :M, 0] - mx) <= b)
            se = np.exp(r - mx[:, None]).sum(1)  # every logit and the maximum move by <= b: each term within e^(+-2b)
            assert np.all(np.abs(part[t, :M, 1] - se) <= se * (np.expm1(2 * b) + 1e-5))
            rows = np.flatnonzero((tc >= 0) & (tc < r.shape[1]))
            assert np.all(np.abs(part[t, rows, 2] - r[rows, tc[rows]]) <= b[rows])
            assert np.all(np.isneginf(np.delete(part[t, :M, 2], rows)))
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


@pytest.mark.parametrize("waves", [4, 8])
def test_rows_independent_of_shape(hip, waves):
    """a row's result depends on the waves only: bit-identical across M, row blocks and column tiles"""
    outs = []
    for M, rb, ct in ((64, 4, 2), (64, 1, 1), (64, 2, 2), (64, 4, 1), (33, 1, 1), (1, 1, 1)):
        out = _launch(hip, hip.HPA_FEPI_RESID, M, 768, 48, waves, rb, ct, True, seed=3)[0]
        outs.append(hip.from_frag(out["frag"], M, 48).view(np.uint32))
    assert all(np.array_equal(o, outs[0][:o.shape[0]]) for o in outs[1:])


@pytest.mark.parametrize("field,value", [("variant", 5), ("ln_fold_c1", 16), ("w_scale", None), ("K", 96)])
def test_refusals(hip, field, value):
    rc = _launch(hip, hip.HPA_FEPI_GELU, 16, 192, 16, 4, 1, 1, True, seed=1, mutate=lambda g: setattr(g, field, value))
    assert rc != 0 and hip.lib().hpa_last_error().decode().strip()
