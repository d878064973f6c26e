"""The fused log-softmax epilogue (HPA_FEPI_SCORE), hpa_score_final and
hpa_logprob_rows against the float64 reference (tests/score_ref64.py).

The SCORE GEMM never stores its logits, so each case runs HPA_FEPI_LOGITS and
HPA_FEPI_SCORE with the same waves, row_blocks, col_tiles and variant on the
same operands: both epilogues see the same fp32 values (one summation order),
and the LOGITS output x is what the float64 reference reads.

  top_id   == the first argmax of x, exactly
  logprob  within 4e-6 + 2^-22 * max(|lse64(x)|, |x[t]|) of x[t] - lse64(x)

Source of the bound (the implemented order, hpa_gemm_body.h / hpa_score.hip):
a tile's sum is four lanes' sums of four terms in [0, 1], combined as
(q0 + q1) + (q2 + q3): at most 5 dependent fp32 additions, bounded as 16
(16 * 2^-24 = 9.5e-7 relative); each term is v_exp_f32((v - m) * log2 e): 1
ulp (1.2e-7) plus the product's rounding, |d| e^d 2^-24 <= 2.2e-8 of the
largest term per term (3.5e-7 over 16): below 1.5e-6 relative on S >= 1,
hence absolute on log S; the tiles are combined in double; lse and the
difference are each rounded to fp32 once (2 * 2^-24 * magnitude).  The bound
is the issue's, not widened; measured worst: 0.08 of it.
"""
import ctypes

import numpy as np
import pytest

import score_ref64 as sr

pytestmark = pytest.mark.gpu


def _stats_tiles(x, Mp):
    M, C = x.shape
    st = np.zeros((C // 16, Mp, 2), np.float32)
    for i in range(C // 16):
        blk = x[:, 16 * i:16 * (i + 1)].astype(np.float64)
        st[i, :M, 0] = blk.sum(1)
        st[i, :M, 1] = (blk * blk).sum(1)
    return st


class _Case:
    """operands on the device (built as test_gpu_fused.py's _run does) and the
    two launches"""

    def __init__(self, hip, M, K, N, seed, w_bf16=False, waves=0, rb=0, ct=0, variant=1, x=None, W=None):
        self.hip, self.L = hip, hip.lib()
        self.M, self.K, self.N, self.Mp = M, K, N, (M + 15) // 16 * 16
        self.shape = (waves, rb, ct, variant)
        rng = np.random.default_rng(seed)
        x = rng.uniform(-1, 1, (M, K)).astype(np.float32) if x is None else x
        W = rng.uniform(-0.05, 0.05, (N, K)).astype(np.float32) if W is None else W
        lw = rng.uniform(0.8, 1.2, K).astype(np.float32)
        lb = rng.uniform(-0.1, 0.1, K).astype(np.float32)
        self.keep = []
        self.x, self.st = self._dev(hip.to_frag(x)), self._dev(_stats_tiles(x, self.Mp))
        self.lw, self.lb = self._dev(lw), self._dev(lb)
        self.w_dtype = hip.HPA_F32
        if w_bf16:
            wb = hip.DeviceBuffer(self.L.hpa_frag_bf16_elems(N, K) * 2)
            self.keep.append(wb)
            hip.check(self.L.hpa_pack_frag_bf16(self._dev(W), N, K, K, wb.ptr), "pack bf16")
            self.w, self.w_dtype = wb.ptr, hip.HPA_BF16
        else:
            self.w = self._dev(hip.to_frag(W))
        self.ntiles = (N + 15) // 16

    def _dev(self, a):
        b = self.hip.DeviceBuffer.from_array(np.ascontiguousarray(a))
        self.keep.append(b)
        return b.ptr

    def _desc(self, epi):
        g = self.hip.HpaFusedGemm()
        g.x, g.M, g.K, g.N = self.x, self.M, self.K, self.N
        g.ln_stats, g.ln_ntiles, g.ln_w, g.ln_b = self.st, self.K // 16, self.lw, self.lb
        g.w, g.w_dtype, g.epilogue = self.w, self.w_dtype, epi
        g.waves, g.row_blocks, g.col_tiles, g.variant = self.shape
        return g

    def logits(self):
        hip = self.hip
        out = hip.DeviceBuffer(self.M * self.N * 4)
        part = hip.DeviceBuffer(self.ntiles * self.Mp * 2 * 4)
        g = self._desc(hip.HPA_FEPI_LOGITS)
        g.out, g.part_out = out.ptr, part.ptr
        hip.check(self.L.hpa_gemm_fused(ctypes.byref(g)), "LOGITS")
        hip.check(self.L.hpa_synchronize())
        return out.download((self.M, self.N))

    def score(self, targets):
        """(logprob, lse, top_id, top_logprob, partials) of one SCORE launch + hpa_score_final"""
        hip, L, M = self.hip, self.L, self.M
        nf = ctypes.c_size_t()
        hip.check(L.hpa_score_workspace(self.N, self.Mp, ctypes.byref(nf)), "workspace")
        part = hip.DeviceBuffer.from_array(np.full(nf.value, np.nan, np.float32))
        g = self._desc(hip.HPA_FEPI_SCORE)
        g.score_target = self._dev(np.asarray(targets, np.int32))
        g.score_part = part.ptr  # g.out stays NULL
        hip.check(L.hpa_gemm_fused(ctypes.byref(g)), "SCORE")
        lp, lse, tlp = (hip.DeviceBuffer(M * 4) for _ in range(3))
        top = hip.DeviceBuffer(M * 4)
        hip.check(L.hpa_score_final(part.ptr, self.ntiles, self.Mp, M, lp.ptr, lse.ptr, top.ptr, tlp.ptr), "final")
        hip.check(L.hpa_synchronize())
        return (lp.download(M), lse.download(M), top.download(M, np.int32), tlp.download(M),
                part.download((self.ntiles, self.Mp, 4)))


def _check(x, targets, lp, lse, top, tlp):
    ref = sr.logprob64(x, targets)
    bound = sr.kernel_bound(x, targets)
    err = np.abs(lp.astype(np.float64) - ref)
    print(f"logprob: worst err {err.max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert np.all(np.isfinite(lp))
    assert np.all(err <= bound), (int(np.argmax(err - bound)), float(err.max()))
    assert np.array_equal(top, sr.first_argmax(x))
    l64 = sr.lse64(x)
    assert np.all(np.abs(lse - l64) <= 4e-6 + 2.0 ** -22 * np.abs(l64))
    am = sr.first_argmax(x)
    assert np.all(np.abs(tlp - sr.logprob64(x, am)) <= sr.kernel_bound(x, am))
    assert np.all(lp[np.asarray(targets) < 0] == 0.0)


def _targets(M, N, seed):
    """column 0, the last column (the partly masked tile when N % 16), both
    sides of a tile boundary, none, then random columns"""
    t = np.random.default_rng(seed).integers(0, N, M).astype(np.int32)
    t[:6] = [0, N - 1, 15, 16, -1, N - (N % 16 or 16)]
    t[M - 1] = N - 1  # the last live row, in the masked tile
    return t


@pytest.mark.parametrize("M,waves,rb,ct,variant", [(37, 0, 0, 0, 1), (37, 4, 1, 1, 0), (37, 16, 1, 1, 1),
                                                   (64, 8, 2, 2, 1), (64, 4, 4, 4, 1), (64, 8, 4, 2, 1)])
def test_score_small_padded_rows_masked_tile(hip, M, waves, rb, ct, variant):
    """(M, K, N) = (37, 128, 1000): 11 padded rows, 8 live columns in the last
    tile; 64 rows carry the multi-row-block / multi-column-tile workgroups"""
    K, N = 128, 1000
    c = _Case(hip, M, K, N, seed=3, waves=waves, rb=rb, ct=ct, variant=variant)
    x = c.logits()
    t = _targets(M, N, 1)
    lp, lse, top, tlp, part = c.score(t)
    _check(x, t, lp, lse, top, tlp)
    # the partials themselves: nothing NaN, padded rows (-inf, 0, -inf, 16 t), the masked tile's sum over 8 columns
    assert not np.isnan(part).any()
    pad = part[:, M:, :]
    assert np.all(pad[..., 0] == -np.inf) and np.all(pad[..., 1] == 0.0) and np.all(pad[..., 2] == -np.inf)
    assert np.array_equal(pad[..., 3].copy().view(np.int32), np.broadcast_to(16 * np.arange(c.ntiles)[:, None],
                                                                           pad.shape[:2]))
    last = x[:, 992:].astype(np.float64)
    assert np.array_equal(part[-1, :M, 0], x[:, 992:].max(-1))
    assert np.all(np.abs(part[-1, :M, 1] - np.exp(last - last.max(-1, keepdims=True)).sum(-1)) <= 1e-5)
    assert np.array_equal(part[0, :M, 0], x[:, :16].max(-1))


def test_score_bf16_small(hip):
    """the looped bf16 kernel (variant 1) and the A-resident one (5) at the small shape"""
    M, K, N = 37, 128, 1000
    for variant, waves, rb, ct in [(1, 8, 1, 1), (1, 4, 2, 2), (5, 8, 1, 0), (5, 4, 1, 2)]:
        c = _Case(hip, M, K, N, seed=4, w_bf16=True, waves=waves, rb=rb, ct=ct, variant=variant)
        x = c.logits()
        t = _targets(M, N, 2)
        _check(x, t, *c.score(t)[:4])


@pytest.mark.parametrize("w_bf16", [False, True])
def test_score_full_vocabulary(hip, w_bf16):
    """(50, 768, 50257), the library's own launch shape, run once per weight type"""
    M, K, N = 50, 768, 50257
    c = _Case(hip, M, K, N, seed=5, w_bf16=w_bf16, variant=0)
    x = c.logits()
    t = _targets(M, N, 3)
    _check(x, t, *c.score(t)[:4])


def test_score_peaked_and_shifted_rows(hip):
    """row 0: one logit about 60 above the rest; row 1: every logit shifted by
    about +300 (expf of the raw value overflows): finite and within the bound"""
    M, K, N = 37, 128, 1000
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.uniform(-0.05, 0.05, (N, K)).astype(np.float32)
    c0 = _Case(hip, M, K, N, seed=6, x=x, W=W)  # its LN weights: the LN'ed A rows, to aim the weights at
    lw = c0.keep[2].download(K)
    lb = c0.keep[3].download(K)
    x64 = x.astype(np.float64)
    ln = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + 1e-5) * lw + lb
    # column 500 += 60 on row 0: add 60 * u0 / |u0|^2 with u0 = LN(row 0); rows 2.. pick up <= ~60 |cos|
    W[500] += (60.0 * ln[0] / (ln[0] @ ln[0])).astype(np.float32)
    # every column += 300 on row 1 (and its projection on the others)
    W += (300.0 * ln[1] / (ln[1] @ ln[1])).astype(np.float32)[None, :]
    c = _Case(hip, M, K, N, seed=6, x=x, W=W)
    xl = c.logits()
    s = np.sort(xl[0])
    assert s[-1] - s[-2] > 50 and xl[1].min() > 250, (s[-1] - s[-2], xl[1].min())
    t = _targets(M, N, 4)
    t[0], t[1] = 500, 7
    lp, lse, top, tlp, _ = c.score(t)
    _check(xl, t, lp, lse, top, tlp)
    assert top[0] == 500 and abs(lp[0]) <= 4e-6 + 2.0 ** -22 * abs(xl[0, 500])
    t[0] = 3  # a token ~60 below the peak
    lp2 = c.score(t)[0]
    _check(xl, t, lp2, lse, top, tlp)
    assert lp2[0] < -50


def test_score_repeats_bit_for_bit(hip):
    c = _Case(hip, 37, 128, 1000, seed=7)
    t = _targets(37, 1000, 5)
    a, b = c.score(t), c.score(t)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.int32), v.view(np.int32))


def test_score_no_target_array(hip):
    """score_target NULL: every row has no target"""
    hip_l = hip.lib()
    c = _Case(hip, 20, 128, 1000, seed=8)
    nf = ctypes.c_size_t()
    hip.check(hip_l.hpa_score_workspace(1000, 32, ctypes.byref(nf)))
    part = hip.DeviceBuffer(nf.value * 4)
    g = c._desc(hip.HPA_FEPI_SCORE)
    g.score_part = part.ptr
    hip.check(hip_l.hpa_gemm_fused(ctypes.byref(g)), "SCORE")
    lp, top = hip.DeviceBuffer(20 * 4), hip.DeviceBuffer(20 * 4)
    hip.check(hip_l.hpa_score_final(part.ptr, 63, 32, 20, lp.ptr, None, top.ptr, None))
    hip.check(hip_l.hpa_synchronize())
    assert np.all(lp.download(20) == 0.0)
    assert np.array_equal(top.download(20, np.int32), sr.first_argmax(c.logits()))


@pytest.mark.parametrize("variant,waves,w_bf16", [(2, 4, False), (3, 1, False), (4, 0, False), (6, 0, False),
                                                   (4, 0, True)])
def test_score_rejected_by_other_variants(hip, variant, waves, w_bf16):
    """one-shot, ring, activation-resident and stream-K refuse the epilogue (nothing is launched)"""
    L = hip.lib()
    c = _Case(hip, 16, 768, 1000, seed=9, w_bf16=w_bf16, waves=waves, variant=variant)
    nf = ctypes.c_size_t()
    hip.check(L.hpa_score_workspace(1000, 16, ctypes.byref(nf)))
    part = hip.DeviceBuffer(nf.value * 4)
    g = c._desc(hip.HPA_FEPI_SCORE)
    g.score_part = part.ptr
    assert L.hpa_gemm_fused(ctypes.byref(g)) != 0
    assert b"SCORE" in L.hpa_last_error()
    g.variant, g.waves, g.score_part = 1, 0, None  # and no partial buffer
    assert L.hpa_gemm_fused(ctypes.byref(g)) != 0


@pytest.mark.parametrize("B,V", [(5, 1000), (3, 50257)])
def test_logprob_rows(hip, B, V):
    """hpa_logprob_rows against lse64 of the rows it was given; rows with
    active <= 0 keep their value"""
    L = hip.lib()
    rng = np.random.default_rng(B + V)
    x = rng.normal(0, 4, (B, V)).astype(np.float32)
    x[0] += 300.0  # shifted row
    x[1, V - 1] = x[1].max() + 60.0  # peaked row, chosen id at the end
    ids = rng.integers(0, V, B).astype(np.int32)
    ids[0], ids[1] = 0, V - 1
    active = np.ones(B, np.int32)
    active[2] = 0
    if B > 3:
        active[3] = -1
    d_x, d_ids, d_act = (hip.DeviceBuffer.from_array(a) for a in (x, ids, active))
    sentinel = np.float32(123.25)
    d_lp = hip.DeviceBuffer.from_array(np.full(B, sentinel, np.float32))
    hip.check(L.hpa_logprob_rows(d_x.ptr, B, V, d_ids.ptr, d_act.ptr, d_lp.ptr), "logprob_rows")
    hip.check(L.hpa_synchronize())
    lp = d_lp.download(B)
    on = active > 0
    err = np.abs(lp.astype(np.float64) - sr.logprob64(x, ids))
    assert np.all(err[on] <= sr.kernel_bound(x, ids)[on]), err
    assert np.all(lp[~on] == sentinel)
    hip.check(L.hpa_logprob_rows(d_x.ptr, B, V, d_ids.ptr, None, d_lp.ptr), "logprob_rows")  # active NULL: every row
    hip.check(L.hpa_synchronize())
    lp2 = d_lp.download(B)
    assert np.all(np.abs(lp2.astype(np.float64) - sr.logprob64(x, ids)) <= sr.kernel_bound(x, ids))
    assert np.array_equal(lp2[on], lp[on])
