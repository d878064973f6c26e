"""Filtered sampling in the decode engine (mode 2): per-sequence temperature /
top-k / top-p read from device memory by the captured step, the setter's
validation, per-slot reseeding, and mode 1 unchanged.

Ids are checked against m.logits() with the pick criterion of
test_gpu_sample_filtered.py (sample_ref64.check_pick_any: the engine does not
expose n_kept, so the id must satisfy c[prev] - tol <= u < c[pick] + tol for an
n the float64 interval admits; tol = sample_ref64.tolerance of that row).
A slot's sampler state is not readable from outside: it is pinned through the
coins the following draws must have used.
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import sample_ref64 as sr
import synth

pytestmark = pytest.mark.gpu

SMALL = dict(maxT=128, V=1000, L=2, NH=2, C=128)
B, PAGE = 6, 16
PARAMS = [(0.0, 0, 1.0), (0.8, 50, 1.0), (1.0, 0, 0.9), (0.5, 10, 0.95), (1.7, 0, 1.0), (1.2, 200, 0.5)]


def _engine(hip, seed=1337, filtered=True, params=PARAMS):
    m = hip.Model(SMALL, params=synth.params(SMALL, seed=3))
    m.decode_init(B, PAGE, SMALL["maxT"])
    m.set_graph(True)
    if params:
        for b, (t, k, p) in enumerate(params):
            m.set_sampling_params(b, t, k, p)
    if seed is not None:
        m.set_sampling(True, seed=seed, filtered=filtered)
    return m


def _check_rows(m, ids, states, params, rows=range(B)):
    """advance the Python streams of `rows` by one coin and check their ids"""
    lg = m.logits()
    for b in rows:
        states[b], u = sr.coin(states[b])
        t, k, p = params[b]
        tol = sr.tolerance(lg[b], t) if t > 0 else 0.0
        sr.check_pick_any(lg[b], t, k, p, u, int(ids[b]), tol)


def test_mode2_step_by_step_with_per_row_settings(hip):
    m = _engine(hip)
    states = [1337 + b for b in range(B)]
    tok = np.random.default_rng(1).integers(0, SMALL["V"], B).astype(np.int32)
    seen = set()
    for s in range(20):
        g = m.step(tok if s == 0 else None)  # sampled ids fed back on the device
        _check_rows(m, g, states, PARAMS)
        assert g[0] == m.logits()[0].argmax()  # the greedy row
        seen.update(int(v) for v in g[1:])
    assert len(seen) > B  # draws, not one id per row
    m.close()


def test_settings_change_under_graph_replay(hip):
    m = _engine(hip)
    states = [1337 + b for b in range(B)]
    params = list(PARAMS)
    tok = np.random.default_rng(2).integers(0, SMALL["V"], B).astype(np.int32)
    for s in range(12):
        if s == 4:  # row 4 greedy from the next step on: no recapture, the kernel reads device memory
            m.set_sampling_params(4, 0.0, 0, 1.0)
            params[4] = (0.0, 0, 1.0)
        if s == 8:  # and back
            m.set_sampling_params(4, 1.7, 0, 1.0)
            params[4] = (1.7, 0, 1.0)
        g = m.step(tok if s == 0 else None)
        _check_rows(m, g, states, params)
        if 4 <= s < 8:
            assert g[4] == m.logits()[4].argmax()
    assert m.sampling_params(4) == pytest.approx((1.7, 0, 1.0))
    m.close()


def test_mode1_is_the_reference_sampler_and_ignores_the_settings(hip):
    m = _engine(hip, seed=None, params=[(0.5, 5, 0.5)] * B)
    m.set_sampling(True, seed=1337)
    sampler = oc.Sampler(B, seed=1337)
    tok = np.random.default_rng(1).integers(0, SMALL["V"], B).astype(np.int32)
    for s in range(12):
        g = m.step(tok if s == 0 else None)
        want = sampler.sample(m.logits())
        assert np.array_equal(g, want), (s, g, want)
    m.close()


def test_ragged_prefill_leaves_an_empty_row_alone(hip):
    params = [(1.0, 0, 1.0)] * B
    m = _engine(hip, params=params)
    states = [1337 + b for b in range(B)]
    rng = np.random.default_rng(4)
    g0 = m.prefill_ragged([rng.integers(0, SMALL["V"], 3 + b) for b in range(B)])
    _check_rows(m, g0, states, params)
    pos0 = m.positions()
    seqs = [rng.integers(0, SMALL["V"], 2) for _ in range(B)]
    seqs[3] = []
    g1 = m.prefill_ragged(seqs)
    assert g1[3] == g0[3] and m.positions()[3] == pos0[3]  # next id and position untouched
    assert np.array_equal(np.delete(m.positions(), 3), np.delete(pos0, 3) + 2)
    _check_rows(m, g1, states, params, rows=[b for b in range(B) if b != 3])
    g2 = m.step(None)  # row 3 draws its SECOND coin here: its state did not advance in the prefill
    _check_rows(m, g2, states, params)
    m.close()


def test_seed_sequence_restarts_one_stream(hip):
    params = [(1.0, 0, 1.0)] * B
    m = _engine(hip, params=params)
    states = [1337 + b for b in range(B)]
    tok = np.random.default_rng(6).integers(0, SMALL["V"], B).astype(np.int32)
    for s in range(3):
        _check_rows(m, m.step(tok if s == 0 else None), states, params)
    m.seed_sequence(2, 999)
    states[2] = 999  # a fresh stream for row 2, the others go on
    for s in range(6):
        _check_rows(m, m.step(None), states, params)
    with pytest.raises(RuntimeError):
        m.seed_sequence(B, 1)
    with pytest.raises(RuntimeError):
        m.seed_sequence(-1, 1)
    m.close()


def test_validation_changes_nothing(hip):
    m = _engine(hip, seed=None, params=None)
    with pytest.raises(RuntimeError):  # no sampler states before set_sampling
        m.seed_sequence(0, 5)
    assert all(m.sampling_params(b) == (1.0, 0, 1.0) for b in range(B))  # the defaults
    m.set_sampling_params(2, 0.7, 40, 0.9)
    before = [m.sampling_params(b) for b in range(B)]
    assert before[2] == pytest.approx((0.7, 40, 0.9)) and before[1] == (1.0, 0, 1.0)
    bad = [dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
           dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(seq=B), dict(seq=-2)]
    for kw in bad:
        args = dict(seq=2, temperature=0.5, top_k=3, top_p=0.5)
        args.update(kw)
        with pytest.raises(RuntimeError):
            m.set_sampling_params(**args)
        assert [m.sampling_params(b) for b in range(B)] == before, kw
    with pytest.raises(RuntimeError):
        m.sampling_params(B)
    m.set_sampling_params(-1, 0.25, 7, 0.5)  # every row
    assert all(m.sampling_params(b) == (0.25, 7, 0.5) for b in range(B))
    t, k = hip.ctypes.c_float(), hip.ctypes.c_int()  # each out pointer is nullable
    hip.check(hip.lib().gpt2_decode_sampling_params(m.h, 1, hip.ctypes.byref(t), None, None))
    hip.check(hip.lib().gpt2_decode_sampling_params(m.h, 1, None, hip.ctypes.byref(k), None))
    assert (t.value, k.value) == (0.25, 7)
    m.close()


def test_release_and_fork_keep_a_slots_settings(hip):
    m = _engine(hip)
    states = [1337 + b for b in range(B)]
    rng = np.random.default_rng(9)
    _check_rows(m, m.prefill_ragged([rng.integers(0, SMALL["V"], 20) for _ in range(B)]), states, PARAMS)
    before = [m.sampling_params(b) for b in range(B)]
    m.release(1)
    assert [m.sampling_params(b) for b in range(B)] == before
    m.fork(0, 1)
    assert [m.sampling_params(b) for b in range(B)] == before
    # slot 1 continues greedy slot 0's prompt with its own settings and its own stream (second coin)
    _check_rows(m, m.step(None), states, PARAMS)
    m.close()
