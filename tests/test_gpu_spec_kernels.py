"""The kernels of speculative sampling against their float64 / Python-integer
restatements (sample_ref64.py, spec_ref64.py):

  hpa_sample_filtered_prob  (n_kept, cut) by sample_ref64.check_cut and equal to
                            hpa_sample_filtered's bit for bit; w_target /
                            w_total within sample_ref64.tolerance(x, T) of the
                            float64 mass over the kept set the device reported,
                            exactly 0 outside it; the masses of a whole row sum
                            to w_total exactly; launches repeat bit for bit
  hpa_sample_filtered_ex    exclude = -1: hpa_sample_filtered bit for bit;
                            excluding the plain pick: check_pick on the
                            residual cdf with the same tolerance
  hpa_spec_accept           exact against the integer walk
"""
import numpy as np
import pytest

import sample_ref64 as sr
import spec_ref64 as sp

pytestmark = pytest.mark.gpu

U64 = np.uint64


def _settings(V):
    """one (T, k, P) per sequence: T in {0, .5, 1, 2}, k in {0, 1, 7, V}, P in {1, .9, 1e-6}"""
    rows = [(1.0, 0, 1.0), (0.5, 7, 1.0), (2.0, 0, 0.9), (0.0, 7, 0.9), (1.0, 7, 0.9), (0.5, 0, 1e-6),
            (2.0, V, 1.0), (1.0, 1, 1.0), (0.5, V, 0.9), (2.0, 7, 1e-6), (0.0, 0, 1.0), (1.0, 0, 0.9)]
    return (np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int32),
            np.array([r[2] for r in rows], np.float32))


def _rows(V, R, rng):
    """quantised logits (tie groups everywhere); where the row is long enough
    five distinct values on top and a group of four equal ones right below, so
    a k = 7 cut falls inside the group; every fourth row all zeros with a few
    -0.0 (a P = 0.9 cut inside one tie group, at the value with two encodings)"""
    x = (np.round(rng.standard_normal((R, V)) * 4) / 4).astype(np.float32)
    for r in range(R):
        if r % 4 == 3:
            x[r] = 0.0
            x[r, rng.integers(0, V, 3)] = -0.0
        elif V >= 64:
            at = rng.choice(V, 9, replace=False)
            top = x[r].max()
            x[r, at[:5]] = top + 1 + np.arange(5, dtype=np.float32)
            x[r, at[5:]] = top + 0.5
    return x


def _targets(x, T, k, P, r):
    """an id of kind r % 7: argmax, interior kept, kept lowest-index tie at the
    cut, tie at the cut that is not kept, below the cut, 0, V - 1 (falling back
    to the argmax where the row has no such id)"""
    V = x.size
    am = int(np.argmax(x))
    kept, n, cut = sp.kept_set(x, T, k, P)
    ties = np.flatnonzero(x == cut)
    kind = r % 7
    if kind == 1 and kept.size > 2:
        return int(kept[kept.size // 2])
    if kind == 2:
        kt = np.intersect1d(ties, kept)
        return int(kt[0]) if kt.size else am
    if kind == 3:
        out = np.setdiff1d(ties, kept)
        return int(out[0]) if out.size else am
    if kind == 4:
        below = np.flatnonzero(x < cut)
        return int(below[below.size // 2]) if below.size else am
    if kind == 5:
        return 0
    if kind == 6:
        return V - 1
    return am


class _Prob:
    def __init__(self, hip, x, seq, T, k, P, tgt, pad=0):
        R, V = x.shape
        self.hip, self.R, self.V = hip, R, V
        # pad floats in front: with pad = 1 (and any V) the first row base is 4-byte aligned only
        self.x = hip.DeviceBuffer(4 * (R * V + pad))
        self.x.upload(x, offset=4 * pad)
        self.xptr = self.x.ptr + 4 * pad
        self.seq = hip.DeviceBuffer.from_array(np.asarray(seq, np.int32)) if seq is not None else None
        self.T = hip.DeviceBuffer.from_array(np.asarray(T, np.float32))
        self.k = hip.DeviceBuffer.from_array(np.asarray(k, np.int32))
        self.P = hip.DeviceBuffer.from_array(np.asarray(P, np.float32))
        self.tgt = hip.DeviceBuffer.from_array(np.asarray(tgt, np.int32))
        self.nk = hip.DeviceBuffer.from_array(np.full(R, -9, np.int32))
        self.cut = hip.DeviceBuffer.from_array(np.full(R, -123.0, np.float32))
        self.wt = hip.DeviceBuffer.from_array(np.full(R, 77, U64))
        self.ws = hip.DeviceBuffer.from_array(np.full(R, 78, U64))

    def launch(self):
        h = self.hip
        h.check(h.lib().hpa_sample_filtered_prob(self.xptr, self.R, self.V, self.seq.ptr if self.seq else None,
                                                 self.T.ptr, self.k.ptr, self.P.ptr, self.tgt.ptr, self.nk.ptr,
                                                 self.cut.ptr, self.wt.ptr, self.ws.ptr), "hpa_sample_filtered_prob")
        R = self.R
        return dict(nk=self.nk.download(R, np.int32), cut=self.cut.download(R, np.float32),
                    wt=self.wt.download(R, U64), ws=self.ws.download(R, U64))


class _Draw:
    """hpa_sample_filtered / _ex on rows x with per-row settings"""

    def __init__(self, hip, x, T, k, P, seeds, pad=0):
        R, V = x.shape
        self.hip, self.R, self.V = hip, R, V
        self.x = hip.DeviceBuffer(4 * (R * V + pad))
        self.x.upload(x, offset=4 * pad)
        self.xptr = self.x.ptr + 4 * pad
        self.T = hip.DeviceBuffer.from_array(np.asarray(T, np.float32))
        self.k = hip.DeviceBuffer.from_array(np.asarray(k, np.int32))
        self.P = hip.DeviceBuffer.from_array(np.asarray(P, np.float32))
        self.seeds = np.asarray(seeds, U64)

    def launch(self, exclude="plain"):
        h, R = self.hip, self.R
        st = h.DeviceBuffer.from_array(self.seeds)
        nxt = h.DeviceBuffer.from_array(np.full(R, -5, np.int32))
        nk = h.DeviceBuffer.from_array(np.full(R, -9, np.int32))
        cut = h.DeviceBuffer.from_array(np.full(R, -123.0, np.float32))
        if isinstance(exclude, str):
            h.check(h.lib().hpa_sample_filtered(self.xptr, R, self.V, self.T.ptr, self.k.ptr, self.P.ptr, st.ptr,
                                                nxt.ptr, None, None, None, nk.ptr, cut.ptr), "hpa_sample_filtered")
        else:
            ex = h.DeviceBuffer.from_array(np.asarray(exclude, np.int32)) if exclude is not None else None
            h.check(h.lib().hpa_sample_filtered_ex(self.xptr, R, self.V, self.T.ptr, self.k.ptr, self.P.ptr, st.ptr,
                                                   nxt.ptr, None, None, None, nk.ptr, cut.ptr,
                                                   ex.ptr if ex else None), "hpa_sample_filtered_ex")
        return dict(next=nxt.download(R, np.int32), nk=nk.download(R, np.int32), cut=cut.download(R, np.float32),
                    st=st.download(R, U64))


def _same(a, b, keys):
    for key in keys:
        assert a[key].tobytes() == b[key].tobytes(), key


# ------------------------------------------------------------ hpa_sample_filtered_prob
@pytest.mark.parametrize("V,R", [(1, 1), (1, 3), (5, 3), (5, 40), (1027, 1), (1027, 40), (50257, 3), (50257, 40)])
def test_prob_masses_cuts_and_repeatability(hip, V, R):
    rng = np.random.default_rng(1000 * R + V)
    x = _rows(V, R, rng)
    Ts, ks, Ps = _settings(V)
    S = Ts.size
    seq = np.array([(5 * r + 1) % S for r in range(R)], np.int32)  # several rows per sequence once R > 12
    tgt = np.array([_targets(x[r], Ts[seq[r]], ks[seq[r]], Ps[seq[r]], r) for r in range(R)], np.int32)
    pad = 1 if V % 2 == 0 or R == 1 else 0  # odd V: rows 1.. are 4-byte aligned already; else shift the base
    dev = _Prob(hip, x, seq, Ts, ks, Ps, tgt, pad=pad)
    out = dev.launch()
    _same(out, dev.launch(), ("nk", "cut", "wt", "ws"))

    # the sampler on the same rows and settings: n_kept and cut bit for bit
    draw = _Draw(hip, x, Ts[seq], ks[seq], Ps[seq], np.arange(R, dtype=U64) + U64(17), pad=pad).launch()
    _same(out, draw, ("nk", "cut"))

    zero_at_unkept_tie = 0
    for r in range(R):
        T, k, P = Ts[seq[r]], int(ks[seq[r]]), Ps[seq[r]]
        n, cut, wt, ws, d = int(out["nk"][r]), out["cut"][r], int(out["wt"][r]), int(out["ws"][r]), int(tgt[r])
        if T == 0:
            assert n == 1 and cut == x[r].max()
            assert (wt, ws) == ((1, 1) if d == int(np.argmax(x[r])) else (0, 1)), (r, d, wt, ws)
            continue
        tol = sr.tolerance(x[r], T)
        sr.check_cut(x[r], T, k, P, n, cut, tol)
        kept = sr.kept_indices(x[r], n, cut)
        assert kept.size == n
        assert 0 < ws < 1 << 62 and 0 <= wt <= ws
        want = sp.accept_prob_kept(x[r], T, kept, d)
        if d not in kept:
            assert wt == 0, (r, d, wt)
            zero_at_unkept_tie += x[r][d] == cut
        else:
            assert abs(wt / ws - want) <= tol, (r, d, wt / ws, want, tol)
        if n == 1:
            assert wt in (0, ws)
    if V >= 64 and R == 40:
        assert zero_at_unkept_tie > 0  # the planted groups put a tie at the cut outside the kept set


def test_prob_without_seq_reads_row_settings_and_bad_targets_have_no_mass(hip):
    V, R = 1027, 12
    x = _rows(V, R, np.random.default_rng(3))
    Ts, ks, Ps = _settings(V)
    tgt = np.array([-1, V, V + 5, -7, 0, 1, 2, 3, 4, 5, 6, 7], np.int32)
    out = _Prob(hip, x, None, Ts, ks, Ps, tgt).launch()
    draw = _Draw(hip, x, Ts, ks, Ps, np.arange(R, dtype=U64) + U64(5)).launch()
    _same(out, draw, ("nk", "cut"))
    assert (out["wt"][:4] == 0).all() and (out["ws"] > 0).all()


@pytest.mark.parametrize("T,k,P", [(1.0, 0, 1.0), (0.7, 50, 0.9), (2.0, 0, 0.9), (0.5, 7, 1.0)])
def test_prob_masses_of_a_whole_row_sum_to_the_total_exactly(hip, T, k, P):
    V = 257
    row = _rows(V, 1, np.random.default_rng(257))
    x = np.repeat(row, V, axis=0)
    out = _Prob(hip, x, np.zeros(V, np.int32), [T], [k], [P], np.arange(V, dtype=np.int32)).launch()
    assert (out["nk"] == out["nk"][0]).all() and (out["ws"] == out["ws"][0]).all()
    n, cut = int(out["nk"][0]), out["cut"][0]
    kept = sr.kept_indices(row[0], n, cut)
    assert kept.size == n
    wt = [int(w) for w in out["wt"]]
    assert sum(wt[i] for i in kept) == int(out["ws"][0])
    assert all(wt[i] == 0 for i in range(V) if i not in kept)


# ------------------------------------------------------------ hpa_sample_filtered_ex
def _ex_case(hip, V, R, seed):
    rng = np.random.default_rng(seed)
    x = _rows(V, R, rng)
    Ts, ks, Ps = _settings(V)
    sel = np.arange(R) % Ts.size
    T, k, P = Ts[sel], ks[sel], Ps[sel]
    seeds = np.arange(R, dtype=U64) * U64(2654435761) + U64(seed + 1)
    return x, T, k, P, seeds, _Draw(hip, x, T, k, P, seeds)


@pytest.mark.parametrize("V,R", [(1, 3), (5, 12), (1027, 24), (50257, 24)])
def test_ex_without_an_exclusion_is_the_plain_sampler_bit_for_bit(hip, V, R):
    x, T, k, P, seeds, dev = _ex_case(hip, V, R, 7 + V)
    plain = dev.launch()
    _same(plain, dev.launch(exclude=None), ("next", "st", "nk", "cut"))
    _same(plain, dev.launch(exclude=np.full(R, -1, np.int32)), ("next", "st", "nk", "cut"))


def _check_excluded_rows(x, T, k, P, seeds, plain, out, excl):
    for r in range(x.shape[0]):
        s, u = sr.coin(int(seeds[r]))
        assert int(out["st"][r]) == s
        n, cut, nxt, d = int(out["nk"][r]), out["cut"][r], int(out["next"][r]), int(excl[r])
        assert n == plain["nk"][r] and out["cut"][r].tobytes() == plain["cut"][r].tobytes()  # the filter, not the removal
        if T[r] == 0:
            assert nxt == int(np.argmax(x[r]))  # greedy rows ignore the exclusion
            continue
        kept = sr.kept_indices(x[r], n, cut)
        if d not in kept:
            assert nxt == plain["next"][r], (r, nxt, plain["next"][r])
        elif n == 1:
            assert nxt == d  # removal would empty the set: dropped
        else:
            assert nxt != d and nxt in kept, (r, nxt, d)
            sp.check_pick_residual(x[r], T[r], n, cut, d, u, nxt, sr.tolerance(x[r], T[r]))


@pytest.mark.parametrize("V,R", [(5, 12), (1027, 24), (50257, 24)])
def test_ex_excluding_the_plain_pick_draws_from_the_residual(hip, V, R):
    x, T, k, P, seeds, dev = _ex_case(hip, V, R, 11 + V)
    plain = dev.launch()
    excl = plain["next"].copy()
    out = dev.launch(exclude=excl)
    _check_excluded_rows(x, T, k, P, seeds, plain, out, excl)
    _same(out, dev.launch(exclude=excl), ("next", "st", "nk", "cut"))


@pytest.mark.parametrize("V,R", [(1027, 24), (50257, 12)])
def test_ex_exclusion_outside_the_kept_set_changes_nothing(hip, V, R):
    x, T, k, P, seeds, dev = _ex_case(hip, V, R, 13 + V)
    plain = dev.launch()
    excl = np.zeros(R, np.int32)
    for r in range(R):
        kept = sr.kept_indices(x[r], int(plain["nk"][r]), plain["cut"][r]) if T[r] > 0 else np.arange(0)
        out = np.setdiff1d(np.arange(V), kept)
        excl[r] = out[len(out) // 2] if out.size and T[r] > 0 else V + 3 + r  # everything kept: an id outside [0, V)
    _same(plain, dev.launch(exclude=excl), ("next", "st", "nk", "cut"))


def test_ex_every_row_of_4096_five_token_rows(hip):
    V, R = 5, 4096
    rng = np.random.default_rng(4096)
    x = (np.round(rng.standard_normal((R, V)) * 2) / 2).astype(np.float32)
    T = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), R)
    k = rng.choice(np.array([0, 2, 3, 5], np.int32), R)
    P = rng.choice(np.array([1.0, 0.9, 0.5], np.float32), R)
    seeds = rng.integers(1, 1 << 63, R, dtype=np.uint64)
    dev = _Draw(hip, x, T, k, P, seeds)
    plain = dev.launch()
    excl = plain["next"].copy()
    out = dev.launch(exclude=excl)
    _check_excluded_rows(x, T, k, P, seeds, plain, out, excl)


# ------------------------------------------------------------ hpa_spec_accept
@pytest.mark.parametrize("kind", ["generic", "zero", "total", "mixed"])
def test_spec_accept_is_the_integer_walk(hip, kind):
    rng = np.random.default_rng({"generic": 1, "zero": 2, "total": 3, "mixed": 4}[kind])
    B = 70  # two workgroups
    lens = np.array([(0, 1, 2, 8)[b % 4] for b in range(B)], np.int32)
    nd = np.maximum(lens - 1, 0)
    draft0 = (np.cumsum(nd) - nd).astype(np.int32)
    ND = int(nd.sum())
    row0 = (np.cumsum(lens) - lens).astype(np.int32)
    start = rng.integers(0, 500, B).astype(np.int32)
    drafts = rng.integers(0, 50257, ND).astype(np.int32)
    ws = rng.integers(1, 1 << 62, ND, dtype=np.uint64)
    frac = {"generic": rng.random(ND), "zero": np.zeros(ND), "total": np.ones(ND),
            "mixed": rng.choice([0.0, 1.0, 0.5, 0.999], ND)}[kind]
    wt = np.array([int(w) if f == 1.0 else int(int(w) * f) for w, f in zip(ws, frac)], U64)
    seeds = rng.integers(1, 1 << 63, B, dtype=np.uint64)
    pos0 = np.full(B, -3, np.int32)

    D = hip.DeviceBuffer.from_array
    d_wt, d_ws, d_dr, d_d0, d_st, d_r0, d_ln = D(wt), D(ws), D(drafts), D(draft0), D(start), D(row0), D(lens)
    d_state, d_pos = D(seeds), D(pos0)
    d_acc, d_cont, d_ex = D(np.full(B, 55, np.int32)), D(np.full(B, 55, np.int32)), D(np.full(B, 55, np.int32))
    hip.check(hip.lib().hpa_spec_accept(d_wt.ptr, d_ws.ptr, d_dr.ptr, d_d0.ptr, d_st.ptr, d_r0.ptr, d_ln.ptr, B,
                                        d_state.ptr, d_acc.ptr, d_cont.ptr, d_ex.ptr, d_pos.ptr), "hpa_spec_accept")
    acc, cont, ex = (b.download(B, np.int32) for b in (d_acc, d_cont, d_ex))
    state, pos = d_state.download(B, U64), d_pos.download(B, np.int32)
    outcomes = set()
    for b in range(B):
        if lens[b] == 0:
            assert (acc[b], cont[b], ex[b], pos[b]) == (-1, -1, -1, -3) and state[b] == seeds[b]
            continue
        sl = slice(draft0[b], draft0[b] + nd[b])
        st, a, rej, coins = sp.accept_walk(int(seeds[b]), wt[sl], ws[sl], drafts[sl])
        assert (int(acc[b]), int(cont[b]), int(ex[b]), int(pos[b])) == (a, row0[b] + a, rej, start[b] + a), b
        assert int(state[b]) == st and len(coins) == min(a + 1, nd[b])
        outcomes.add("all" if rej < 0 else "first" if a == 0 else "middle")
    if kind == "zero":
        assert (acc[lens > 1] == 0).all()
    if kind == "total":
        assert np.array_equal(acc[lens > 0], nd[lens > 0]) and (ex[lens > 0] == -1).all()
    if kind == "generic":
        assert outcomes == {"all", "first", "middle"}
