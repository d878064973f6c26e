"""The float64 restatement of filtered sampling (sample_ref64.py) on hand-made
rows with known answers, its agreement with the reference driver's sampler
(oracle_ctypes.Sampler) where no filter is set, and the library's new
exports.  No GPU."""
import ctypes

import numpy as np
import pytest

import oracle_ctypes as oc
import sample_ref64 as sr


def test_canonical_order_and_topk_ties():
    #             0    1    2    3    4    5    6    7
    x = np.array([1.0, 3.0, 2.0, 3.0, 2.0, 2.0, 0.0, 3.0], np.float32)
    row = sr.Row(x, 1.0, 4)
    assert list(row.order) == [1, 3, 7, 2, 4, 5, 0, 6]
    assert row.K == 4
    # k = 4 cuts the tie group {2, 4, 5} after its lowest index
    assert list(sr.kept_indices(x, 4, row.cut(4))) == [1, 2, 3, 7]
    assert row.cut(4) == 2.0
    # k = 5 takes the two lowest-indexed of the group
    row5 = sr.Row(x, 1.0, 5)
    assert list(sr.kept_indices(x, 5, row5.cut(5))) == [1, 2, 3, 4, 7]
    # k = 0 and k >= V keep everything
    assert sr.Row(x, 1.0, 0).K == 8 and sr.Row(x, 1.0, 8).K == 8 and sr.Row(x, 1.0, 15).K == 8


def test_top_p_prefix_and_ties_at_the_cut():
    # masses 8 : 4 : 2 : 1 : 1 over 16 (at indices 3, 0, 4, 1, 2), the rest negligible
    x = np.full(9, -80.0, np.float32)
    x[[3, 0, 4, 1, 2]] = np.log(np.array([8.0, 4.0, 2.0, 1.0, 1.0])).astype(np.float32)
    row = sr.Row(x, 1.0, 0)
    assert list(row.order[:5]) == [3, 0, 4, 1, 2]
    np.testing.assert_allclose(row.M[:5], [0.5, 0.75, 0.875, 0.9375, 1.0], atol=1e-6)
    assert row.n_kept(0.4) == 1 and row.n_kept(0.6) == 2 and row.n_kept(0.8) == 3
    # the cut falls inside the tie {1, 2}: one of them suffices for 0.9, the lowest index
    assert row.n_kept(0.9) == 4
    assert list(sr.kept_indices(x, 4, row.cut(4))) == [0, 1, 3, 4]
    assert row.n_kept(0.95) == 5
    assert row.n_kept(1e-6) == 1          # at least one token
    assert row.n_kept(1.0) == 9           # P = 1 keeps the whole set
    assert sr.Row(x, 1.0, 3).n_kept(1.0) == 3
    # top-p is taken inside the top-k set: masses 8 : 4 over 12
    r2 = sr.Row(x, 1.0, 2)
    np.testing.assert_allclose(r2.M, [2 / 3, 1.0], atol=1e-6)
    assert r2.n_kept(0.6) == 1 and r2.n_kept(0.7) == 2


def test_draw_walks_kept_tokens_in_index_order():
    x = np.full(8, -80.0, np.float32)
    x[[3, 0, 4, 1, 2]] = np.log(np.array([8.0, 4.0, 2.0, 1.0, 1.0])).astype(np.float32)
    # P = 0.8 keeps {3, 0, 4}; in index order 0, 3, 4 with masses 4 : 8 : 2 over 14
    for u, want in [(0.0, 0), (0.28, 0), (0.29, 3), (0.85, 3), (0.86, 4), (0.999, 4)]:
        got, n, cut = sr.pick(x, 1.0, 0, 0.8, np.float32(u))
        assert (got, n) == (want, 3), (u, got, n)
        assert cut == x[4]
    # k = 1 and greedy give the argmax whatever the coin
    for u in (0.0, 0.5, 0.99):
        assert sr.pick(x, 1.0, 1, 1.0, np.float32(u))[:2] == (3, 1)
        assert sr.pick(x, 0.0, 0, 1.0, np.float32(u))[:2] == (3, 1)
    # ties for the maximum: lowest index
    y = np.array([1.0, 5.0, 5.0, 0.0, 5.0, 2.0, 1.0, 1.0, 3.0, 5.0], np.float32)
    assert sr.pick(y, 0.0, 0, 1.0, np.float32(0.7))[0] == 1
    assert sr.pick(y, 1.0, 1, 1.0, np.float32(0.7))[0] == 1
    # k = 2 over four equal maxima keeps indices 1 and 2, half each
    assert sr.pick(y, 1.0, 2, 1.0, np.float32(0.49))[0] == 1
    assert sr.pick(y, 1.0, 2, 1.0, np.float32(0.51))[0] == 2


def test_temperature_peaks_and_flattens():
    x = np.array([0.0, 1.0, 2.0, 3.0, 2.5, 1.5, 0.5, -1.0, 2.0], np.float32)
    # T -> 0+: all the mass on the maximum, any P keeps one token
    row = sr.Row(x, 0.01, 0)
    assert row.M[0] > 1 - 1e-12 and row.n_kept(0.999) == 1
    assert sr.pick(x, 0.01, 0, 0.999, np.float32(0.97))[0] == 3
    # T large: close to uniform, P = 0.5 needs five of nine
    assert sr.Row(x, 1e4, 0).n_kept(0.5) == 5
    # temperature never changes the order or the top-k set
    assert list(sr.Row(x, 0.3, 4).order) == list(sr.Row(x, 3.0, 4).order)


def test_sanitise_and_coin():
    assert sr.sanitise(-1.0, -3, 0.0) == (1.0, 0, 1.0)
    assert sr.sanitise(float("nan"), 5, 1.5) == (1.0, 5, 1.0)
    assert sr.sanitise(float("inf"), 0, float("nan")) == (1.0, 0, 1.0)
    # the Python generator is the reference's random_f32
    L = oc.lib()
    st = ctypes.c_ulonglong(1337)
    s = 1337
    for _ in range(50):
        s, u = sr.coin(s)
        assert u == np.float32(L.oracle_random_f32(ctypes.byref(st))) and s == st.value


def _logits(kind, B, V, rng):
    if kind == "randn40":
        return (rng.standard_normal((B, V)) * 40).astype(np.float32)
    x = (rng.standard_normal((B, V)) - 30).astype(np.float32)  # spike
    x[np.arange(B), rng.integers(0, V, B)] = 5.0
    return x


# seeds fixed here; a seed whose coin lands within the tolerance of a cdf
# boundary is replaced by the next one, here on the CPU
@pytest.mark.parametrize("kind,seed", [("randn40", 1337), ("spike", 4242)])
def test_unfiltered_picks_equal_the_reference_sampler(kind, seed):
    B, V, draws = 4, 50257, 3
    x = _logits(kind, B, V, np.random.default_rng(11))
    tol = [sr.tolerance(x[b], 1.0) for b in range(B)]
    for attempt in range(8):
        states = [seed + 1000 * attempt + b for b in range(B)]
        ok = True
        for _ in range(draws):
            for b in range(B):
                states[b], u = sr.coin(states[b])
                c = sr.index_cdf(x[b], np.arange(V), 1.0)
                ok = ok and np.abs(c - float(u)).min() > tol[b]
        if ok:
            break
    assert ok, "no seed keeps every coin clear of the cdf boundaries"
    base = seed + 1000 * attempt
    sampler = oc.Sampler(B, seed=base)
    states = [base + b for b in range(B)]
    for _ in range(draws):
        want = sampler.sample(x)
        for b in range(B):
            states[b], u = sr.coin(states[b])
            got, n, cut = sr.pick(x[b], 1.0, 0, 1.0, u)
            assert got == want[b] and n == V and cut == x[b].min(), (b, got, want[b])
    assert states == [s.value for s in sampler.states]


def test_library_exports_filtered_sampling():
    """the library loads without a GPU and exposes the new entry points"""
    import pagedattn
    L = pagedattn.lib()
    for name in ("hpa_sample_filtered", "gpt2_decode_set_sampling_params", "gpt2_decode_sampling_params",
                 "gpt2_decode_seed_sequence"):
        assert getattr(L, name).argtypes is not None, name
