"""The numpy restatement of the shared-prefix decode attention
(tests/shared_ref64.py) against the float64 reference of tests/attn_ref64.py,
its case set and its mutations.  CPU only.

The unmutated cascade (prefix partials per split, the suffix partial, the
merge) stays within REF_WORST of the reference at every split count of the GPU
test; each mutation of shared_ref64.MUTATIONS -- the prefix dropped, the
prefix one tile short, a merge that does not rescale, a member reading
another member's query, a neutral record written with m = 0 -- exceeds BAR
(tests/test_attn_ref64.py) on the case built for it.
"""
import numpy as np
import pytest

import attn_ref64 as ar
import shared_ref64 as sr
from test_attn_ref64 import BAR, REF_WORST

_cache = {}


def _cases(P=16):
    if P not in _cache:
        _cache[P] = sr.shared_cases(P)
        _cache[P].cs.reference()
    return _cache[P]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


@pytest.mark.parametrize("splits", sr.SPLITS)
def test_cascade_unmutated_within_ref_worst(splits):
    sc = _cases()
    r = sc.cs.ratios(sr.cascade_outputs(sc, splits))
    by = sc.cs.worst_by_kind(r)
    print(f"SHAREDREF cascade splits={splits} rows={sc.B} " + " ".join(f"{k}={v:.3f}" for k, v in by.items()))
    assert r.max() <= REF_WORST, by
    assert by["below_floor_all"] == 0.0


CAUGHT_BY = {"drop_prefix": "hot", "prefix_short_one_tile": "hot", "merge_no_rescale": "ramp_up",
             "other_members_q": "hot", "neutral_m_zero": "below_floor_one"}


@pytest.mark.parametrize("mutate", sr.MUTATIONS)
def test_mutations_exceed_the_bar(mutate):
    sc = _cases()
    splits = 3  # two tiles over three ranges: one range has no tile (neutral_m_zero needs it)
    r = sc.cs.ratios(sr.cascade_outputs(sc, splits, mutate))
    by = sc.cs.worst_by_kind(r)
    print(f"SHAREDREF mutation {mutate}: " + " ".join(f"{k}={v:.3g}" for k, v in by.items()))
    assert by[CAUGHT_BY[mutate]] > BAR, by
    # rows outside every unit are untouched by any of them
    assert r[sc.unit_of < 0].max() <= REF_WORST


def test_case_set_covers_what_it_claims():
    sc = _cases()
    cs = sc.cs
    sizes = sorted(len(m) for m, _ in sc.units)
    assert {1, 2, 3, 8} <= set(sizes)
    assert {t for _, t in sc.units} == {1, 2, 5}
    kinds = {k for ks in cs.kind for k in ks}
    assert kinds == set(ar.KINDS)
    offs = set()
    for m, t in sc.units:
        for i in m:
            assert 64 * t <= sc.pos[i] and sc.own_from[i] >= 64 * t  # the kernels' invariant
            offs.add(int(sc.pos[i]) - 64 * t)
        # members sit apart by index: some other row lies between the first and the last
        if len(m) >= 2:
            assert max(m) - min(m) + 1 > len(m)
        g = {int(sc.group[i]) for i in m}
        assert len(g) == 1 and -1 not in g
    assert {0, 63, 64, 300} <= offs
    # two units over the same pages
    by_group = {}
    for u, (m, t) in enumerate(sc.units):
        by_group.setdefault(int(sc.group[m[0]]), []).append(u)
    assert any(len(u) == 2 for u in by_group.values())
    # a unit whose tiles lie below what two of its members share between themselves
    assert any(sorted(int(sc.own_from[i]) // 64 for i in m)[-2] > t for m, t in sc.units if len(m) >= 3)
    # members of a group hold equal K, V below the tokens they share
    for a in range(sc.B):
        for b in range(a + 1, sc.B):
            if sc.group[a] >= 0 and sc.group[a] == sc.group[b]:
                n = min(sc.own_from[a], sc.own_from[b])
                assert np.array_equal(cs.seqs[a][0][:n], cs.seqs[b][0][:n])
                assert np.array_equal(cs.seqs[a][1][:n], cs.seqs[b][1][:n])
    assert (sc.unit_of < 0).sum() >= 5
    # hot keys reach 0, 64t - 1, 64t and pos of some member
    out, unit, E, wmax = cs.reference()
    hits = set()
    for i in range(sc.B):
        if cs.kind[i][0] == "hot" and sc.unit_of[i] >= 0:
            t = int(sc.skip[i])
            for h in range(ar.NH):
                c = slice(h * ar.HS, (h + 1) * ar.HS)
                j = int(np.argmax(cs.seqs[i][0][:, c] @ cs.q[i, c]))
                hits.add("0" if j == 0 else "64t-1" if j == 64 * t - 1 else "64t" if j == 64 * t
                         else "pos" if j == sc.pos[i] else "edge")
    assert {"0", "64t-1", "64t", "pos", "edge"} <= hits


def test_plan_restatement_on_the_worked_examples():
    P = 16
    # 64 forks of one prompt at position 1000: 62 full shared pages, 15 tiles, 8 units of 8
    n = 1000 // P
    bt = np.full((64, 64), -1, np.int32)
    bt[:, :n] = np.arange(n)
    bt[:, n] = 1000 + np.arange(64)  # the copied tail page, private
    pos = np.full(64, 1000)
    units, skip = sr.plan(bt, pos, P)
    assert len(units) == 8 and all(len(m) == 8 and t == 15 for m, t in units)
    assert units[0][0] == list(range(8)) and (skip == 15).all()
    sr.check_invariants(bt, pos, P, units)
    # forks of slot 0 at 128 and at 640 tokens, all three past 700
    bt = np.full((3, 64), -1, np.int32)
    bt[0, :50] = np.arange(50)
    bt[1, :8], bt[1, 8:50] = np.arange(8), 100 + np.arange(42)
    bt[2, :40], bt[2, 40:50] = np.arange(40), 200 + np.arange(10)
    pos = np.array([710, 720, 730])
    units, skip = sr.plan(bt, pos, P)
    assert units == [([0, 2], 10)] and skip.tolist() == [10, 0, 10]
