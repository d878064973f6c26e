"""CPU self-test of tests/pick_inputs.py: the conditions on the inputs (on the
float64 products and the CPU oracle alone, no kernel), and each checker fed
numpy-made wrong answers of the kinds a broken pick would give:

  * a pad column (id N) holding 0.0 wins a row whose logits are all negative
  * the highest tied column wins instead of the lowest
  * the ids of rows 0 and 1 are swapped
  * an inactive row is written

and the correct numpy-made answers, which every checker accepts.  This is how
the GPU tests (test_gpu_pick_edges.py, test_gpu_pick_engine.py) are shown to
bite; no mutated kernel runs anywhere.
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import pick_inputs as pi
from gemm_bounds import rbf16

SHAPES = [(64, 768, 9601), (64, 1600, 2001)]


def _partials(x, N, Mp, owner=None, P=None, pad_value=-np.inf, last_wins=False):
    """(P, Mp, 2) partials of logits x (M, N), made the slow plain way: per
    partial a scan over its columns in ascending order with strict > (>= when
    last_wins); pad columns hold pad_value; rows >= M: (-inf, first column)"""
    M = x.shape[0]
    ntiles = (N + 15) // 16
    owner = np.arange(ntiles) if owner is None else np.asarray(owner)
    P = ntiles if P is None else P
    xp = np.full((M, ntiles * 16), pad_value, np.float32)
    xp[:, :N] = x
    val = np.full((P, Mp), -np.inf, np.float32)
    col = np.full((P, Mp), pi.EMPTY, np.int32)
    for p in range(P):
        cols = np.concatenate([np.arange(16 * t, 16 * t + 16) for t in np.flatnonzero(owner == p)] or
                              [np.zeros(0, np.int64)]).astype(np.int64)
        if pad_value == -np.inf:
            cols = cols[cols < N]
        for c in cols:
            take = xp[:, c] >= val[p, :M] if last_wins else xp[:, c] > val[p, :M]
            val[p, :M][take] = xp[take, c]
            col[p, :M][take] = c
    out = np.zeros((P, Mp, 2), np.float32)
    out[..., 0] = val
    out[..., 1] = col.view(np.float32)
    return out


def _reduce(part):
    """hpa_argmax_final's rule on partials: the largest value, the lowest column among equals"""
    val, col = part[..., 0], part[..., 1].copy().view(np.int32).astype(np.int64)
    best = val.max(0)
    return np.where(val == best[None, :], col, np.int64(1) << 40).min(0)


@pytest.fixture(scope="module")
def small_shifted():
    """a narrow stand-in for the checkers' own tests: N = 16 * 20 + 1"""
    inp = pi.shifted(37, 768, 321, seed=1)
    return inp, inp["acc"].astype(np.float32)


@pytest.mark.parametrize("M,K,N", SHAPES + [(64, 768, 50257)])
def test_shifted_inputs_meet_their_condition(M, K, N):
    inp = pi.shifted(M, K, N, seed=K + N)
    mx, distinct, margin, bound = pi.check_shifted_inputs(inp)
    print(f"shifted K={K} N={N}: max {mx:.2f}, {distinct} distinct ids of {M}, "
          f"smallest margin {margin:.3e}, worst bound {bound:.2e}")
    assert inp["x"].dtype == np.float32 and abs(inp["x"].mean()) < 0.01  # x itself is untouched: zero-mean
    # a pad column's accumulator (0.0) would beat every row
    assert np.all(inp["acc"].max(-1) < 0.0)


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_shifted_inputs_bf16_meet_their_condition(M, K, N):
    inp = pi.shifted(M, K, N, seed=K + N, w_bf16=True)
    mx, distinct, margin, bound = pi.check_shifted_inputs(inp)
    print(f"shifted bf16 K={K} N={N}: max {mx:.2f}, {distinct} distinct, margin {margin:.3e}, bound {bound:.2e}")


def test_shifted_refuses_the_small_k():
    """K = 128: the shift is too small (the issue's figure: a maximum near -0.1)"""
    with pytest.raises(AssertionError):
        pi.check_shifted_inputs(pi.shifted(64, 128, 1009, seed=3))


@pytest.mark.parametrize("M,K,N", SHAPES)
@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_ties_inputs_meet_their_condition(M, K, N, which):
    E, O = pi.tie_sets(N)[which]
    inp = pi.ties(M, K, N, E, O)
    pi.check_ties_inputs(inp)
    x32 = inp["acc"].astype(np.float32)
    pi.check_tied_logits(x32, inp)
    assert np.array_equal(inp["want"][:2], [min(E), min(O)])
    pi.check_pick(inp["want"], x32, N)
    assert np.all(inp["x"].sum(-1) == 0)  # zero-mean exactly
    # dyadic: bf16 keeps every weight
    assert np.array_equal(rbf16(inp["W"][:, :4]), inp["W"][:, :4])
    if which == "a":  # what the set is there for
        assert {7, 9} <= set(E) and 16 in E and N - 1 in E and N - 1 in O and (N - 1) % 16 == 0
        assert any(e + 1 in E and e % 16 == 0 for e in E)


def test_checkers_accept_right_answers(small_shifted):
    inp, x = small_shifted
    M, N = x.shape
    Mp, ntiles = 48, 21
    for owner, P in ((None, None), (pi.tile_owner_strided(ntiles, 8), 8), (pi.tile_owner_runs(ntiles, 8), 8),
                     (pi.tile_owner_runs(ntiles, 21), 24)):  # 24: three partials own nothing
        part = _partials(x, N, Mp, owner, P)
        pi.check_partials(part, x, N, M, owner)
        pi.check_pick(_reduce(part)[:M], x, N)
    assert np.array_equal(pi.tile_owner_runs(21, 8), np.repeat(np.arange(8), [3, 3, 3, 3, 3, 2, 2, 2]))
    # rows >= M of the looped kernel: (-inf, the tile's first column)
    part = _partials(x, N, Mp)
    part[:, M:, 1] = (16 * np.arange(ntiles, dtype=np.int32)).view(np.float32)[:, None]
    pi.check_partials(part, x, N, M)
    t = pi.ties(37, 768, 321, [7, 9, 16, 160, 161, 319, 320], [9, 23, 161, 320])
    xt = t["acc"].astype(np.float32)
    for owner, P in ((None, None), (pi.tile_owner_strided(ntiles, 8), 8), (pi.tile_owner_runs(ntiles, 8), 8)):
        part = _partials(xt, N, Mp, owner, P)
        pi.check_partials(part, xt, N, M, owner)
        ids = _reduce(part)[:M]
        pi.check_pick(ids, xt, N)
        assert np.array_equal(ids, t["want"])


def test_rejects_a_pad_column_that_wins(small_shifted):
    """the mask lost on the value that feeds the maximum: the last tile's 15
    pad columns hold the accumulator of zero weights, 0.0, above every logit"""
    inp, x = small_shifted
    M, N = x.shape
    part = _partials(x, N, 48, pad_value=0.0)
    assert np.all(part[-1, :M, 0] == 0.0) and np.all(part[-1, :M, 1].copy().view(np.int32) == N)
    ids = _reduce(part)[:M]
    assert np.all(ids == N)
    with pytest.raises(AssertionError):
        pi.check_partials(part, x, N, M)
    with pytest.raises(AssertionError):
        pi.check_pick(ids, x, N)
    # the same with the column reported inside the vocabulary (value unmasked, index clamped)
    part[-1, :M, 1] = np.int32(N - 1).view(np.float32)
    with pytest.raises(AssertionError):
        pi.check_partials(part, x, N, M)
    with pytest.raises(AssertionError):
        pi.check_pick(_reduce(part)[:M], x, N)
    # on uniform operands the same mistake is invisible: the maximum is positive
    rng = np.random.default_rng(0)
    pos = (pi.ln64(rng.uniform(-1, 1, (M, 768)), 1.0, 0.0) @ rng.uniform(-0.05, 0.05, (N, 768)).T).astype(np.float32)
    pi.check_pick(_reduce(_partials(pos, N, 48, pad_value=0.0))[:M], pos, N)


def test_rejects_the_highest_tied_column():
    M, N = 37, 321
    t = pi.ties(M, 768, N, [7, 9, 16, 160, 161, 319, 320], [9, 23, 161, 320])
    x = t["acc"].astype(np.float32)
    part = _partials(x, N, 48, last_wins=True)  # >= in the scan: the last equal column of every tile
    with pytest.raises(AssertionError):
        pi.check_partials(part, x, N, M)
    # a right scan inside the tiles, the reducer taking the highest column among equal tiles
    good = _partials(x, N, 48)
    val, col = good[..., 0], good[..., 1].copy().view(np.int32)
    ids = np.where(val == val.max(0)[None, :], col, -1).max(0)[:M]
    assert np.array_equal(ids[:2], [320, 320])
    with pytest.raises(AssertionError):
        pi.check_pick(ids, x, N)
    # per-workgroup partials visited in slot order, the first slot kept on equal values: with strided
    # ownership slot order is not column order: column 23 is tile 1 -> slot 1, column 130 is tile 8 -> slot 0
    t = pi.ties(M, 768, N, [23, 130], [23, 130])
    x = t["acc"].astype(np.float32)
    owner = pi.tile_owner_strided(21, 8)
    pw = _partials(x, N, 48, owner, 8)
    pi.check_partials(pw, x, N, M, owner)
    first_slot = pw[..., 1].copy().view(np.int32)[pw[..., 0].argmax(0), np.arange(48)][:M]
    assert np.all(first_slot == 130) and np.all(t["want"] == 23)
    with pytest.raises(AssertionError):
        pi.check_pick(first_slot, x, N)
    pi.check_pick(_reduce(pw)[:M], x, N)


def test_rejects_swapped_rows(small_shifted):
    inp, x = small_shifted
    M, N = x.shape
    ids = x.argmax(-1)
    assert ids[0] != ids[1]
    pi.check_pick(ids, x, N)
    ids[[0, 1]] = ids[[1, 0]]
    with pytest.raises(AssertionError):
        pi.check_pick(ids, x, N)
    part = _partials(x, N, 48)
    part[:, [0, 1]] = part[:, [1, 0]]
    with pytest.raises(AssertionError):
        pi.check_partials(part, x, N, M)
    t = pi.ties(4, 768, 321, [0], [320])
    with pytest.raises(AssertionError):
        pi.check_pick(t["want"][[1, 0, 2, 3]], t["acc"].astype(np.float32), 321)


def test_rejects_a_written_inactive_row_and_finite_padded_rows(small_shifted):
    inp, x = small_shifted
    M, N = x.shape
    active = np.array([1, 0, -1, 1, 2], np.int32)
    before = np.full(5, -7, np.int32)
    after = before.copy()
    after[[0, 3, 4]] = [5, 6, 7]
    pi.check_untouched(active, before, after)
    pi.check_untouched(None, before, after)
    for row in (1, 2):
        bad = after.copy()
        bad[row] = 9
        with pytest.raises(AssertionError):
            pi.check_untouched(active, before, bad)
    part = _partials(x, N, 48)
    part[3, M, 0] = -5.0  # a padded row holding a finite value
    with pytest.raises(AssertionError):
        pi.check_partials(part, x, N, M)
    part = _partials(x, N, 48)
    part[3, 2, 1] = np.int32(pi.EMPTY).view(np.float32)  # the empty marker beside a finite value
    with pytest.raises(AssertionError):
        pi.check_partials(part, x, N, M)


@pytest.mark.parametrize("C,NH,V,delta,beta,T", [(128, 2, 1000, 0.03, 1.0, 24), (768, 12, 5009, 0.01, 1.5, 24)])
def test_negative_logit_params_meet_their_condition(C, NH, V, delta, beta, T):
    """the oracle's logits on the fixture: every one <= -1, at least 8 greedy
    ids over 3 x T random tokens; no embedding row's mean moves"""
    import synth
    cfgd = dict(maxT=64, V=V, L=2, NH=NH, C=C)
    p0, p = synth.params(cfgd, seed=7), pi.negative_logit_params(cfgd, 7, delta, beta)
    w0, w1 = p0[:V * C].reshape(V, C).astype(np.float64), p[:V * C].reshape(V, C).astype(np.float64)
    assert np.abs(w1.mean(-1) - w0.mean(-1)).max() <= 2.0 ** -24  # only the roundings of the adds
    changed = np.flatnonzero(p != p0)
    assert changed.min() >= 0 and np.all((changed < V * C) | (changed >= p.size - C))  # wte and lnfb only
    orc = oc.PagedDecoder(p, oc.cfg(64, V, 2, NH, C), 3, 16, 64)
    rng = np.random.default_rng(7)
    rows = np.stack([orc.step(rng.integers(0, V, 3).astype(np.int32))[1].copy() for _ in range(T)])
    orc.close()
    lo, hi, distinct = pi.check_negative_regime(rows)
    print(f"C={C} V={V} delta={delta} beta={beta}: logits in [{lo:.1f}, {hi:.1f}], {distinct} distinct greedy ids")
    with pytest.raises(AssertionError):  # today's weights: the regime the suite already covers
        o2 = oc.PagedDecoder(p0, oc.cfg(64, V, 2, NH, C), 3, 16, 64)
        r2 = np.stack([o2.step(rng.integers(0, V, 3).astype(np.int32))[1].copy() for _ in range(4)])
        o2.close()
        pi.check_negative_regime(r2)
