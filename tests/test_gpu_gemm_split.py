"""hpa_gemm_fused variant 7 (hpa_gemm_split.hip): fp32 weights on the bf16 MFMA by exact operand splitting.

Held to float64 under the project's fp32 bar, gemm_bounds.fp32_bound on the true operands (not bf16-rounded),
LayerNorm'ed in float64; the folded LN under the folded form's own fp32 bar (test_gpu_fused.test_fused_ln_fold:
the epilogue computes rstd * (acc - mean * c1), so the fp32 error scales with rstd (|x||W'| + |mean||c1|)).
"""
import ctypes

import numpy as np
import pytest

from gemm_bounds import fp32_bound
from test_gpu_fused import _gelu_tanh, _ln, _stats_tiles

pytestmark = pytest.mark.gpu
ROWS = 128  # a row is the same at every M <= ROWS


def _launch(hip, epi, ln, M, K, N, waves, rb, ct, pool=None, ops=None, mutate=None):
    """one variant-7 launch -> (downloads by name, float64 reference with bias, bound); ops: (x, W) given;
    mutate: the descriptor is changed first and only the status comes back"""
    rng = np.random.default_rng(K + N)
    x = rng.uniform(-1, 1, (ROWS, K)).astype(np.float32)[:M]
    W = rng.uniform(-0.05, 0.05, (N, K)).astype(np.float32)
    if ops:
        x, W = ops
    bias = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    lw, lb = rng.uniform(0.8, 1.2, K).astype(np.float32), rng.uniform(-0.1, 0.1, K).astype(np.float32)
    res = rng.uniform(-1, 1, (ROWS, N)).astype(np.float32)[:M]
    Mp, ntn, L = (M + 15) // 16 * 16, (N + 15) // 16, hip.lib()
    keep, out, tgt, bt, pos = [], {}, None, None, None

    def dev(a):
        keep.append(hip.DeviceBuffer.from_array(np.ascontiguousarray(a)))
        return keep[-1].ptr

    def buf(name, n):
        out[name] = hip.DeviceBuffer(n * 4)
        return out[name].ptr

    g = hip.HpaFusedGemm()
    g.x, g.M, g.K, g.N, g.w, g.w_dtype = dev(hip.to_frag(x)), M, K, N, dev(hip.to_frag(W)), hip.HPA_F32
    g.waves, g.row_blocks, g.col_tiles, g.variant, g.epilogue = waves, rb, ct, 7, epi
    bare = epi in (hip.HPA_FEPI_LOGITS, hip.HPA_FEPI_SCORE)
    a = x.astype(np.float64)
    if not bare:
        g.bias = dev(bias)
    if ln != "none":
        g.ln_stats, g.ln_ntiles, g.ln_w, g.ln_b = dev(_stats_tiles(x, Mp)), K // 16, dev(lw), dev(lb)
        a = _ln(a, lw, lb)
    bound = fp32_bound(a, W)
    if ln == "fold":  # the weights packed with the LN folded in (hpa_ln_fold_pack)
        wf, c1, c2 = hip.DeviceBuffer(L.hpa_frag_elems(N, K) * 4), hip.DeviceBuffer(N * 4), hip.DeviceBuffer(N * 4)
        keep.extend([wf, c1, c2])
        hip.check(L.hpa_ln_fold_pack(dev(W), N, K, g.ln_w, g.ln_b, g.bias, wf.ptr, c1.ptr, c2.ptr), "fold")
        g.w, g.bias, g.ln_fold_c1 = wf.ptr, c2.ptr, c1.ptr
        x64, Wg = x.astype(np.float64), (W * lw).astype(np.float64)
        mu = x64.mean(-1)
        rstd = 1 / np.sqrt(((x64 - mu[:, None]) ** 2).mean(-1) + 1e-5)
        bound = np.maximum(bound, 4e-6 * rstd[:, None] * (np.abs(x64) @ np.abs(Wg).T + np.abs(mu)[:, None] * np.abs(Wg.sum(1))) + 2e-6)
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
        return L.hpa_gemm_fused(ctypes.byref(g))
    hip.check(L.hpa_gemm_fused(ctypes.byref(g)), "gemm_fused")
    hip.check(L.hpa_synchronize())
    out = {k: v.download(v.nbytes // 4) for k, v in out.items()}
    out.update(res=res, tgt=tgt, bt=bt, pos=pos)
    acc = a @ W.astype(np.float64).T
    return out, acc if bare else acc + bias, bound


# epilogue (QKVb / QKV8: a bf16 / fp8 pool), LN, M, K, N, waves, row blocks, column tiles.  K = 32: one step, fewer
# than the waves; 96: 3 steps, ragged over 4 and 8; 160: 5, odd.  M = 17: a ragged row block; 65: five row groups
# (4 row blocks fall to 1); 64 / 128: one / two groups of 4 row blocks.  N = 40: a partial tile (row-major outputs
# only); 80: 5 tiles, the last group of 2 or 4 runs past N; 16 at col_tiles 2 / 4: a group wholly past it but one.
CASES = [("RESID", "none", 1, 32, 16, 4, 1, 1), ("RESID", "load", 17, 96, 80, 8, 4, 2), ("RESID", "fold", 65, 160, 80, 4, 4, 4),
         ("RESID", "fold", 128, 160, 80, 4, 4, 4), ("RESID", "none", 64, 96, 16, 8, 4, 2), ("RESID", "load", 1, 160, 16, 8, 1, 1),
         ("GELU", "load", 17, 160, 80, 4, 1, 1), ("GELU", "fold", 64, 96, 80, 8, 4, 2), ("GELU", "none", 65, 32, 16, 8, 4, 4),
         ("GELU", "fold", 1, 32, 80, 4, 4, 2), ("LOGITS", "none", 17, 96, 40, 4, 4, 2), ("LOGITS", "load", 65, 160, 40, 8, 1, 1),
         ("LOGITS", "load", 64, 32, 80, 4, 4, 4), ("SCORE", "load", 17, 160, 40, 8, 4, 2), ("SCORE", "none", 128, 96, 80, 4, 4, 4),
         ("SCORE", "load", 1, 32, 16, 4, 1, 1), ("QKV", "load", 17, 96, 384, 4, 1, 1), ("QKV", "fold", 65, 160, 384, 8, 4, 2),
         ("QKVb", "none", 64, 32, 384, 4, 4, 4), ("QKV8", "load", 17, 160, 384, 8, 4, 2)]


@pytest.mark.parametrize("epi,ln,M,K,N,waves,rb,ct", CASES)
def test_kernel_against_float64(hip, epi, ln, M, K, N, waves, rb, ct):
    dt = {"QKV": hip.HPA_F32, "QKVb": hip.HPA_BF16, "QKV8": hip.HPA_FP8}.get(epi)
    pool = hip.Pool(1, 2, 16, 4 * M, dtype=dt) if dt is not None else None
    out, ref, bound = _launch(hip, getattr(hip, "HPA_FEPI_" + epi.rstrip("b8")), ln, M, K, N, waves, rb, ct, pool)
    Mp, ntn = (M + 15) // 16 * 16, (N + 15) // 16
    if epi == "RESID":
        got = hip.from_frag(out["frag"], Mp, N)
        assert np.all(np.abs(got[:M] - (out["res"] + ref)) <= bound + 1e-6) and np.all(got[M:] == 0)
        g16 = got[:M].astype(np.float64).reshape(M, ntn, 16)  # stats: the sums of what was stored (test_gpu_fused's bar)
        st = out["stats"].reshape(ntn, Mp, 2)[:, :M]
        assert np.all(np.abs(st[..., 0].T - g16.sum(-1)) <= 2.0 ** -19 * np.abs(g16).sum(-1))
        assert np.all(np.abs(st[..., 1].T - (g16 ** 2).sum(-1)) <= 2.0 ** -19 * (g16 ** 2).sum(-1))
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
        # the pool's format on a value within the bound of ref: bf16 RNE half an ulp (2^-8 relative); e4m3 (scale 1)
        # of the clamped value 2^-4 relative or 2^-10 below 2^-6
        fmt = {"QKV": 0.0, "QKVb": 2.0 ** -8 * (np.abs(ref) + bound), "QKV8": 2.0 ** -4 * np.abs(ref) + 2.0 ** -10}[epi]
        want = np.clip(ref, -448, 448) if epi == "QKV8" else ref
        for b in range(M):
            k, v = pool.read_tokens(0, out["bt"][b], out["pos"][b] + 1)
            got = np.concatenate([k[out["pos"][b]], v[out["pos"][b]]])
            assert np.all(np.abs(got - want[b, C:]) <= (bound + fmt)[b, C:])


@pytest.mark.parametrize("onehot", ["W", "A"])
@pytest.mark.parametrize("waves,rb,ct", [(4, 1, 1), (8, 4, 2)])
def test_single_products_pin_the_six_terms(hip, onehot, waves, rb, ct):
    """K = 32, LOGITS (the bare product), one operand with a single nonzero per row: every output is ONE fp32
    product a w of full 24-bit mantissas (normal deviates), |out - a w| <= 2^-20 |a||w|.  Derivation: with
    |mid| < 2^-7 |x| and |lo| < 2^-15 |x| the three products left out, (mid, lo) (lo, mid) (lo, lo), are below
    (2 * 2^-22 + 2^-30) |a||w|; the six kept are exact in fp32 and enter the accumulator one MFMA each, the first
    into zero, so five fp32 roundings of a partial sum <= |a||w|: 5 * 2^-24.  Together 13.004 * 2^-24 < 2^-20.  The
    other waves fold zeros.  A kernel without (mid, mid), (lo, hi) or (hi, lo) is off by up to 2^-14 or 2^-15."""
    rng = np.random.default_rng(7)
    M, N, K = 64, 80, 32
    full, hot = rng.standard_normal((N, K)).astype(np.float32), np.zeros((M, K), np.float32)
    hot[np.arange(M), rng.integers(0, K, M)] = rng.standard_normal(M).astype(np.float32)
    x, W = (hot, full) if onehot == "A" else (full[:M], np.vstack([hot, hot[:N - M]]))
    out, ref, _ = _launch(hip, hip.HPA_FEPI_LOGITS, "none", M, K, N, waves, rb, ct, ops=(x, W))
    mag = np.abs(x.astype(np.float64)) @ np.abs(W.astype(np.float64)).T  # one term per output
    err = np.abs(out["rows"].reshape(M, N) - ref)
    print("worst |out - ref| / |a||w| in units of 2^-24:", float((err / np.maximum(mag, 1e-300)).max() * 2 ** 24))
    assert np.all(err <= 2.0 ** -20 * mag)


@pytest.mark.parametrize("waves", [4, 8])
def test_rows_independent_of_shape(hip, waves):
    """a row's bits depend on the waves only: identical across M, row blocks and column tiles"""
    outs = []
    for M, rb, ct in ((128, 4, 4), (128, 4, 2), (64, 1, 1), (64, 2, 2), (65, 4, 1), (17, 1, 2), (33, 2, 4), (1, 1, 1)):
        out = _launch(hip, hip.HPA_FEPI_RESID, "load", M, 160, 80, waves, rb, ct)[0]
        outs.append(hip.from_frag(out["frag"], M, 80).view(np.uint32))
    assert all(np.array_equal(o, outs[0][:o.shape[0]]) for o in outs[1:])


@pytest.mark.parametrize("field,value,says", [("w_dtype", "HPA_BF16", "w_dtype"), ("K", 48, "K % 32"), ("waves", 16, "waves")])
def test_refusals(hip, field, value, says):  # each with its own message and nothing launched
    value = getattr(hip, value) if isinstance(value, str) else value
    rc = _launch(hip, hip.HPA_FEPI_GELU, "load", 16, 96, 16, 4, 1, 1, mutate=lambda g: setattr(g, field, value))
    err = hip.lib().hpa_last_error().decode()
    assert rc != 0 and "variant 7" in err and says in err
