"""tests/top_ref64.py against a brute-force selection on hand-made rows: the
reference of the GPU tests is itself pinned on the cases the order rule is
about (ties, signed zeros, the cut inside a tie group, k = 1 and k = V)."""
import numpy as np
import pytest

import score_ref64 as sr
import top_ref64 as tr


def _rows():
    rng = np.random.default_rng(1)
    V = 37
    noise = rng.standard_normal(V).astype(np.float32)
    all_equal = np.full(V, 0.5, np.float32)
    zeros = -np.abs(noise) - 1.0
    zeros[[3, 9, 20, 36]] = np.float32(-0.0)
    zeros[[0, 12, 30]] = np.float32(0.0)
    straddle = noise.copy()
    straddle[[1, 2, 3]] = [9.0, 8.0, 7.0]
    straddle[[35, 5, 17, 6, 29]] = 6.0  # ranks 3..7: a cut at k = 5 falls inside the group
    top_ties = noise.copy()
    top_ties[[36, 0, 18]] = noise.max()
    return dict(noise=noise, all_equal=all_equal, zeros=zeros, straddle=straddle, top_ties=top_ties,
                ramp_up=np.arange(V, dtype=np.float32), ramp_down=-np.arange(V, dtype=np.float32))


@pytest.mark.parametrize("name", sorted(_rows()))
@pytest.mark.parametrize("k", [1, 5, 37])
def test_topk64_is_the_brute_force_selection(name, k):
    x = _rows()[name]
    ids, lps = tr.topk64(x, k)
    assert np.array_equal(ids, tr.topk_brute(x, k))
    assert len(set(ids.tolist())) == k
    assert np.all(np.diff(lps) <= 0)
    assert np.array_equal(lps, x[ids].astype(np.float64) - sr.lse64(x))
    assert ids[0] == sr.first_argmax(x)


def test_hand_checked_rows():
    r = _rows()
    assert tr.topk64(r["all_equal"], 5)[0].tolist() == [0, 1, 2, 3, 4]
    assert np.allclose(tr.topk64(r["all_equal"], 37)[1], -np.log(37.0), rtol=0, atol=1e-14)
    # signed zeros are one value: ordered by column whatever their sign
    assert tr.topk64(r["zeros"], 7)[0].tolist() == [0, 3, 9, 12, 20, 30, 36]
    # three distinct values, then the five-way tie in column order
    assert tr.topk64(r["straddle"], 5)[0].tolist() == [1, 2, 3, 5, 6]
    assert tr.topk64(r["straddle"], 8)[0].tolist() == [1, 2, 3, 5, 6, 17, 29, 35]
    assert tr.topk64(r["ramp_up"], 3)[0].tolist() == [36, 35, 34]
    assert tr.topk64(r["ramp_down"], 3)[0].tolist() == [0, 1, 2]


def test_oracle_alone_has_half_the_ranks_clear():
    """tests/test_gpu_top_logprobs.py compares score_top's ids with the oracle's
    only at clear ranks (the j-th sorted value more than TIE_MARGIN = 1e-3 from
    both neighbours); its seed is chosen so that at least half of all (row,
    rank) pairs are clear.  The same rows, on the CPU oracle alone."""
    import oracle_ctypes as oc
    import synth
    small = dict(maxT=256, V=1000, L=2, NH=2, C=128)
    params = synth.params(small, seed=11)
    lens, pre, k, tie = [37, 0, 20], 5, 5, 1e-3
    rng = np.random.default_rng(6)
    pre_tok = rng.integers(0, 1000, (pre, 3)).astype(np.int32)
    seqs = [rng.integers(0, 1000, n).astype(np.int32) for n in lens]
    n_clear = n_all = 0
    for b in (0, 2):
        orc = oc.PagedDecoder(params, oc.cfg(256, 1000, 2, 2, 128), 1, 16, 256, page_seed=b + 1)
        for t in pre_tok[:, b]:
            orc.step(np.array([t], np.int32))
        rows = np.stack([orc.step(seqs[b][t:t + 1])[1][0].copy() for t in range(lens[b])])
        orc.close()
        s = -np.sort(-rows.astype(np.float64), -1)[:, :k + 1]
        below = (s[:, :-1] - s[:, 1:]) > tie
        above = np.concatenate([np.ones((len(rows), 1), bool), below[:, :-1]], 1)
        n_clear += int((below & above).sum())
        n_all += below.size
    assert 2 * n_clear >= n_all, (n_clear, n_all)


def test_batched_rows_and_bound():
    r = _rows()
    x = np.stack([r["noise"], r["zeros"], r["straddle"]])
    ids, lps = tr.topk64(x, 5)
    for i in range(3):
        a, b = tr.topk64(x[i], 5)
        assert np.array_equal(ids[i], a) and np.array_equal(lps[i], b)
    assert np.array_equal(ids[:, 0], sr.first_argmax(x))
    bd = tr.bound(x, ids)
    assert bd.shape == (3, 5)
    for j in range(5):  # the same bound as score_ref64's at those columns
        assert np.array_equal(bd[:, j], sr.kernel_bound(x, ids[:, j]))
