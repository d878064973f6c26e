"""gpt2_attn_shared_plan (paged_infer.c, pure host code) through ctypes: the
worked examples of paged_infer.h's text, the invariants the kernels rely on
over random fork forests, rewound members, the thresholds, 9 sharers, and
equality with the numpy restatement (tests/shared_ref64.py).  No GPU."""
import numpy as np
import pytest

import pagedattn as hip
import shared_ref64 as sr


def _c_plan(bt, pos, P, min_tiles=1, min_members=2, max_units=None):
    n, members, tiles, skip = hip.attn_shared_plan(bt, pos, P, min_tiles, min_members, max_units)
    units = []
    for u in range(members.shape[0]):
        m = [int(x) for x in members[u] if x >= 0]
        if u < n:
            assert tiles[u] > 0 and m and members[u, :len(m)].tolist() == m  # packed, -1 padded behind
            units.append((m, int(tiles[u])))
        else:
            assert tiles[u] == 0 and not m
    return units, skip


def _forks(n, pos, P, stride=None):
    """n forks of one prompt at `pos` tokens: full pages shared, the tail page private"""
    full = pos // P
    stride = stride or full + 2
    bt = np.full((n, stride), -1, np.int32)
    bt[:, :full] = np.arange(full)
    if pos % P:
        bt[:, full] = 10000 + np.arange(n)
    return bt, np.full(n, pos, np.int32)


def test_worked_example_64_forks():
    bt, pos = _forks(64, 1000, 16)
    units, skip = _c_plan(bt, pos, 16)
    assert len(units) == 8
    for u, (m, t) in enumerate(units):
        assert m == list(range(8 * u, 8 * u + 8)) and t == 15
    assert (skip == 15).all()
    sr.check_invariants(bt, pos, 16, units)


def test_worked_example_two_fork_lengths():
    P = 16
    bt = np.full((3, 64), -1, np.int32)
    bt[0, :50] = np.arange(50)
    bt[1, :8], bt[1, 8:50] = np.arange(8), 100 + np.arange(42)      # forked at 128 tokens
    bt[2, :40], bt[2, 40:50] = np.arange(40), 200 + np.arange(10)   # forked at 640 tokens
    pos = np.array([710, 720, 730], np.int32)
    units, skip = _c_plan(bt, pos, P)
    assert units == [([0, 2], 10)]   # k = 1: 1 * 10 = 10 beats k = 2: 2 * 2 = 4
    assert skip.tolist() == [10, 0, 10]


def _forest(rng, B, P, stride):
    """a random fork forest: slot b is a fresh prompt or a fork of an earlier slot at a random length;
    positions both below and above the shared length"""
    bt = np.full((B, stride), -1, np.int32)
    pos = np.zeros(B, np.int32)
    nxt = 0
    for b in range(B):
        L = int(rng.integers(0, stride * P - 1))
        if b and rng.random() < 0.7:
            src = int(rng.integers(0, b))
            n = int(rng.integers(0, pos[src] + 1))
            full = n // P
            bt[b, :full] = bt[src, :full]
            have = full
            if rng.random() < 0.2:  # rewound below the fork point: the shared pages stay in the table
                L = int(rng.integers(0, n + 1))
            else:
                L = max(L, n)
        else:
            have = 0
        need = (L + P) // P  # pages through position L
        for i in range(have, min(need, stride)):
            bt[b, i] = nxt
            nxt += 1
        pos[b] = min(L, stride * P - 1)
    return bt, pos


@pytest.mark.parametrize("P", [8, 16, 64])
def test_invariants_and_restatement_on_random_forests(P):
    rng = np.random.default_rng([11, P])
    n_units = 0
    for trial in range(40):
        B = int(rng.integers(1, 65))
        stride = int(rng.integers(2, 1200 // P))
        bt, pos = _forest(rng, B, P, stride)
        for min_tiles, min_members in ((1, 2), (2, 2), (1, 3), (3, 4)):
            units, skip = _c_plan(bt, pos, P, min_tiles, min_members)
            sr.check_invariants(bt, pos, P, units)
            for m, t in units:
                assert t >= min_tiles and len(m) >= min_members
            want_units, want_skip = sr.plan(bt, pos, P, min_tiles, min_members)
            assert units == want_units, (trial, min_tiles, min_members)
            assert np.array_equal(skip, want_skip)
            in_unit = {b for m, _ in units for b in m}
            assert all(skip[b] == 0 for b in range(B) if b not in in_unit)
            n_units += len(units)
    assert n_units > 40  # the forests do share


def test_rewound_member_shrinks_or_leaves():
    P = 16
    bt, pos = _forks(4, 1000, P)
    pos[2] = 200   # rewound: 3 whole tiles left under it
    pos[3] = 40    # below one tile: not a candidate at all
    units, skip = _c_plan(bt, pos, P)
    # leader 0: candidates 1 (15 tiles) and 2 (3 tiles); 1 * 15 beats 2 * 3
    assert units == [([0, 1], 15)] and skip.tolist() == [15, 15, 0, 0]
    pos[1] = 200
    units, skip = _c_plan(bt, pos, P)
    assert units == [([0, 1, 2], 3)] and skip.tolist() == [3, 3, 3, 0]
    sr.check_invariants(bt, pos, P, units)


def test_thresholds_filter():
    P = 16
    bt, pos = _forks(3, 200, P)  # 12 full pages: 3 tiles
    assert _c_plan(bt, pos, P, 3, 2)[0] == [([0, 1, 2], 3)]
    assert _c_plan(bt, pos, P, 4, 2)[0] == []
    assert _c_plan(bt, pos, P, 1, 4)[0] == []
    assert _c_plan(bt, pos, P, 1, 3)[0] == [([0, 1, 2], 3)]


def test_nine_sharers_are_eight_and_one():
    bt, pos = _forks(9, 700, 16)
    units, skip = _c_plan(bt, pos, 16)
    assert units == [(list(range(8)), 10)] and skip.tolist() == [10] * 8 + [0]
    bt, pos = _forks(10, 700, 16)
    units, skip = _c_plan(bt, pos, 16)
    assert units == [(list(range(8)), 10), ([8, 9], 10)]


def test_bad_arguments():
    bt, pos = _forks(8, 300, 16)
    with pytest.raises(RuntimeError):
        hip.attn_shared_plan(bt, pos, 16, max_units=3)       # fewer than B / 2
    with pytest.raises(RuntimeError):
        hip.attn_shared_plan(bt, pos, 16, min_tiles=0)
    with pytest.raises(RuntimeError):
        hip.attn_shared_plan(bt, pos, 16, min_members=1)
    with pytest.raises(RuntimeError):
        hip.attn_shared_plan(bt, pos, 0)
    assert hip.attn_shared_plan(bt, pos, 16, max_units=4)[0] == 1
