"""The float64 scoring reference (tests/score_ref64.py) checked on its own, and
hpa_score_workspace (host arithmetic, no device)."""
import ctypes

import numpy as np
import pytest

import score_ref64 as sr


def _rows(seed=0, rows=7, V=1000):
    return np.random.default_rng(seed).normal(0, 3, (rows, V)).astype(np.float32)


def test_probabilities_sum_to_one():
    x = _rows()
    lp = x.astype(np.float64) - sr.lse64(x)[:, None]
    assert np.all(np.abs(np.exp(lp).sum(-1) - 1.0) <= 1e-12)
    assert np.all(lp <= 0)


def test_shift_invariance():
    """log-softmax does not move when the row is shifted by 1e4 (a naive
    exp(x) overflows there)"""
    x = _rows(1).astype(np.float64)
    t = np.arange(x.shape[0]) * 37 % x.shape[1]
    a = sr.logprob64(x, t)
    b = sr.logprob64(x + 1e4, t)
    assert np.all(np.isfinite(b))
    assert np.all(np.abs(a - b) <= 1e-9)  # 1e4 + x carries ~2e-12 of rounding per element


def test_dominant_logit():
    """one logit 60 above the rest: its log-probability is -(V-1) e^-60 = -8.7e-24
    (0 at float64 resolution of the lse), every other column's is -60"""
    V = 1000
    x = np.zeros((1, V), np.float32)
    x[0, 123] = 60.0
    assert sr.first_argmax(x)[0] == 123
    lp = sr.logprob64(x, [123])[0]
    assert lp <= 0 and abs(lp) <= 1e-14
    assert abs(sr.logprob64(x, [5])[0] + 60.0) <= 1e-12


def test_ties_resolve_to_lowest_column():
    x = np.zeros((3, 64), np.float32)
    x[0, [9, 40]] = 2.0
    x[1, [63, 0]] = 1.0
    assert list(sr.first_argmax(x)) == [9, 0, 0]


def test_no_target_is_zero():
    x = _rows(2, rows=3)
    assert list(sr.logprob64(x, [-1, 4, -1])[[0, 2]]) == [0.0, 0.0]


@pytest.fixture(scope="module")
def L():
    import pagedattn
    return pagedattn.lib()


@pytest.mark.parametrize("V,rows,want", [(1000, 16, 63 * 16 * 4), (1000, 1024, 63 * 1024 * 4),
                                         (50257, 1024, 3142 * 1024 * 4), (50257, 16, 3142 * 16 * 4)])
def test_score_workspace(L, V, rows, want):
    n = ctypes.c_size_t()
    assert L.hpa_score_workspace(V, rows, ctypes.byref(n)) == 0
    assert n.value == want


def test_score_workspace_default_chunk_within_64_mib(L):
    """the engine's default chunk (1024 rows) at GPT-2's vocabulary"""
    n = ctypes.c_size_t()
    assert L.hpa_score_workspace(50257, 1024, ctypes.byref(n)) == 0
    assert n.value * 4 <= 64 << 20


@pytest.mark.parametrize("rows", [0, -16, 24, 1000])
def test_score_workspace_rejects_bad_chunk(L, rows):
    n = ctypes.c_size_t(7)
    assert L.hpa_score_workspace(1000, rows, ctypes.byref(n)) != 0
    assert n.value == 7
    assert L.hpa_score_workspace(0, 16, ctypes.byref(n)) != 0
