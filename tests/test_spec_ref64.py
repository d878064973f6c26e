"""The speculative-sampling rule on the CPU (spec_ref64.py): the analytic
identity that makes the emitted token a plain mode-2 draw, hand-built cases of
the integer accept walk, and the new entry points' presence in the library."""
import ctypes

import numpy as np
import pytest

import sample_ref64 as sr
import spec_ref64 as sp


def _row37():
    return (np.random.default_rng(37).standard_normal(37) * 2.5).astype(np.float32)


@pytest.mark.parametrize("T,k,P", [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 5, 1.0), (1.3, 0, 0.9), (0.7, 5, 0.9)])
def test_accept_or_resample_is_a_plain_draw(T, k, P):
    """[y = d] p(d) + (1 - p(d)) residual_d(y) = p(y) for every draft id d"""
    x = _row37()
    V = x.size
    T = float(np.float32(T))  # the settings are fp32 on the device
    kept, n, cut = sp.kept_set(x, T, k, P)
    assert kept.size == n and (k == 0 or n <= k) and (P < 1 or k or n == V)
    p = np.zeros(V)
    p[kept] = sp.masses(x, kept, T)
    assert abs(p.sum() - 1) < 1e-12
    for d in range(V):
        pd = sp.accept_prob(x, T, k, P, d)
        assert pd == pytest.approx(p[d], abs=1e-15)
        rest, c = sp.residual(x, T, kept, d)
        res = np.zeros(V)
        res[rest] = np.diff(np.concatenate([[0.0], c]))
        assert d not in rest or kept.size == 1
        out = (1 - pd) * res
        out[d] += pd
        assert np.abs(out - p).max() <= 1e-12, (d, np.abs(out - p).max())


def test_greedy_row_is_a_point_mass():
    x = _row37()
    am = int(np.argmax(x))
    assert sp.accept_prob(x, 0.0, 5, 0.9, am) == 1.0
    assert all(sp.accept_prob(x, 0.0, 0, 1.0, d) == 0.0 for d in range(x.size) if d != am)


def _coins(state, n):
    out = []
    for _ in range(n):
        state, r = sr.xorshift_u32(state)
        out.append(r >> 8)
    return state, out


def test_walk_all_accept_first_reject_middle_reject():
    seed = 1234
    end3, js = _coins(seed, 3)
    tot = 1 << 40
    above = [(j * tot >> 24) + 1 for j in js]  # the smallest mass with w * 2^24 > tot * j
    below = [w - 1 for w in above]
    assert all(sp.accepts(a, tot, j) and not sp.accepts(b, tot, j) for a, b, j in zip(above, below, js))
    drafts = [11, 22, 33]
    # all accept: three coins, nothing rejected
    st, a, rej, coins = sp.accept_walk(seed, above, [tot] * 3, drafts)
    assert (st, a, rej, coins) == (end3, 3, -1, js)
    # first reject: one coin only
    st, a, rej, coins = sp.accept_walk(seed, [below[0]] + above[1:], [tot] * 3, drafts)
    assert (a, rej, coins) == (0, 11, js[:1]) and st == _coins(seed, 1)[0]
    # middle reject: two coins
    st, a, rej, coins = sp.accept_walk(seed, [above[0], below[1], above[2]], [tot] * 3, drafts)
    assert (a, rej, coins) == (1, 22, js[:2]) and st == _coins(seed, 2)[0]


def test_walk_mass_zero_and_mass_equal_to_the_total():
    for seed in (1, 2, 3, 1 << 63):
        # mass 0: rejected whatever the coin (j = 0 included: 0 > 0 is false)
        assert not sp.accepts(0, 12345, 0)
        _, a, rej, coins = sp.accept_walk(seed, [0], [1 << 50], [7])
        assert (a, rej, len(coins)) == (0, 7, 1)
        # mass == total: accepted whatever the coin (j < 2^24)
        assert sp.accepts(1, 1, (1 << 24) - 1)
        st, a, rej, coins = sp.accept_walk(seed, [1 << 50] * 7, [1 << 50] * 7, list(range(7)))
        assert (a, rej, len(coins)) == (7, -1, 7) and st == _coins(seed, 7)[0]
    # the greedy encoding (1, 1) / (0, 1)
    _, a, rej, _ = sp.accept_walk(5, [1, 1, 0, 1], [1, 1, 1, 1], [4, 5, 6, 7])
    assert (a, rej) == (2, 6)


def test_walk_of_no_drafts_draws_nothing():
    assert sp.accept_walk(99, [], [], []) == (99, 0, -1, [])


def test_new_entry_points_are_exported_and_need_an_engine():
    import pagedattn as pa

    L = pa.lib()
    for name in ("hpa_sample_filtered_prob", "hpa_sample_filtered_ex", "hpa_spec_accept",
                 "gpt2_decode_verify_sampled"):
        assert hasattr(L, name), name
    L.gpt2_alloc.restype = ctypes.c_void_p
    h = ctypes.c_void_p(L.gpt2_alloc())
    assert h
    try:
        nd = np.zeros(4, np.int32)
        acc = np.full(4, 7, np.int32)
        toks = np.full((4, 8), 7, np.int32)
        I = ctypes.POINTER(ctypes.c_int)
        rc = L.gpt2_decode_verify_sampled(h, None, nd.ctypes.data_as(I), acc.ctypes.data_as(I),
                                          toks.ctypes.data_as(I), None)
        assert rc != 0
        assert (acc == 7).all() and (toks == 7).all()
    finally:
        L.gpt2_release.argtypes = [ctypes.c_void_p]
        L.gpt2_release(h)
