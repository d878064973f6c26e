"""The kernels of sampled tree speculation:

  hpa_sample_filtered_prob_multi  every mass, total, n_kept and cut equal to
                                  hpa_sample_filtered_prob's for the same (row,
                                  id) bit for bit; scattered through dst;
                                  launches repeat bit for bit
  hpa_sample_filtered_exn         n_exclude 0 / 1: hpa_sample_filtered / _ex bit
                                  for bit; longer lists: check_pick on the
                                  multi-id residual cdf (tree_spec_ref64)
  hpa_spec_tree_accept            exact against the integer walk
"""
import numpy as np
import pytest

import sample_ref64 as sr
import tree_ref64 as tr
import tree_spec_ref64 as ts
from test_gpu_spec_kernels import _Draw, _Prob, _rows, _same, _settings, _targets

pytestmark = pytest.mark.gpu

U64 = np.uint64
NT = ts.NT


# ------------------------------------------------------------ hpa_sample_filtered_prob_multi
def _target_lists(x, Ts, ks, Ps, seq):
    """per row a list of r % 8 ids: the seven kinds of _targets rotated by the
    row, with a repeat (rows 2 mod 3) and an id outside [0, V) (rows 1 mod 3)"""
    R, V = x.shape
    lists = []
    for r in range(R):
        b = seq[r]
        kinds = [_targets(x[r], Ts[b], int(ks[b]), Ps[b], (r + i) % 7) for i in range(7)]
        ids = kinds[:r % 8]
        if len(ids) >= 2 and r % 3 == 2:
            ids[-1] = ids[0]
        if len(ids) >= 2 and r % 3 == 1:
            ids[1] = V + r if r % 2 else -1 - r
        lists.append(ids)
    return lists


@pytest.mark.parametrize("V,pad", [(50257, 0), (1000, 1), (1000, 0), (63, 1)])
def test_prob_multi_is_the_single_target_kernel_bit_for_bit(hip, V, pad):
    R = 12
    rng = np.random.default_rng(100 + V)
    x = _rows(V, R, rng)
    Ts, ks, Ps = _settings(V)
    seq = np.arange(R, dtype=np.int32)
    lists = _target_lists(x, Ts, ks, Ps, seq)
    assert sorted(len(l) for l in lists) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7]
    total = sum(len(l) for l in lists)

    # the only route before this kernel: one duplicated row per (row, id); an extra id 0 per row for n_kept / cut
    pairs = [(r, d) for r in range(R) for d in lists[r] + [0]]
    ref = _Prob(hip, x[[r for r, _ in pairs]], np.array([seq[r] for r, _ in pairs], np.int32), Ts, ks, Ps,
                np.array([d for _, d in pairs], np.int32), pad=pad).launch()

    # dst: a scatter over a larger array, the entries of a row nowhere near each other
    slots = rng.permutation(total + 5)[:total].astype(np.int32)
    tg = np.full((R, NT), 12345, np.int32)  # entries past n_targets are not read as ids
    dst = np.full((R, NT), 0, np.int32)
    at = 0
    for r in range(R):
        for i, d in enumerate(lists[r]):
            tg[r, i], dst[r, i] = d, slots[at]
            at += 1
    nt = np.array([len(l) for l in lists], np.int32)

    D = hip.DeviceBuffer.from_array
    xb = hip.DeviceBuffer(4 * (R * V + pad))
    xb.upload(x, offset=4 * pad)
    d_seq, d_T, d_k, d_P, d_tg, d_nt, d_dst = D(seq), D(Ts), D(ks), D(Ps), D(tg), D(nt), D(dst)

    def launch():
        nk, cut = D(np.full(R, -9, np.int32)), D(np.full(R, -123.0, np.float32))
        wt, ws = D(np.full(total + 5, 77, U64)), D(np.full(total + 5, 78, U64))
        hip.sample_filtered_prob_multi(xb.ptr + 4 * pad, R, V, d_seq.ptr, d_T.ptr, d_k.ptr, d_P.ptr, d_tg.ptr, d_nt.ptr,
                                       d_dst.ptr, nk.ptr, cut.ptr, wt.ptr, ws.ptr)
        return dict(nk=nk.download(R, np.int32), cut=cut.download(R, np.float32), wt=wt.download(total + 5, U64),
                    ws=ws.download(total + 5, U64))

    out = launch()
    _same(out, launch(), ("nk", "cut", "wt", "ws"))
    at = 0
    nonzero = 0
    for p, (r, d) in enumerate(pairs):
        if p + 1 == len(pairs) or pairs[p + 1][0] != r:  # the extra id: the row's n_kept and cut
            assert out["nk"][r] == ref["nk"][p] and out["cut"][r].tobytes() == ref["cut"][p].tobytes(), r
            continue
        s = slots[at]
        at += 1
        assert int(out["wt"][s]) == int(ref["wt"][p]) and int(out["ws"][s]) == int(ref["ws"][p]), (r, d, s)
        if d < 0 or d >= V:
            assert out["wt"][s] == 0
        nonzero += out["wt"][s] > 0
    assert at == total and nonzero > total // 4
    untouched = np.setdiff1d(np.arange(total + 5), slots)
    assert (out["wt"][untouched] == 77).all() and (out["ws"][untouched] == 78).all()


def test_prob_multi_two_rows_of_one_sequence_pack_by_draft(hip):
    """rows 0 and 1 belong to sequence 0 (a root with two children, a child with
    three): their masses land at the sequence's packed drafts, the settings are
    the sequence's, and a negative dst writes nothing"""
    V, R = 1000, 3
    x = _rows(V, R, np.random.default_rng(9))
    Ts, ks, Ps = _settings(V)
    seq = np.array([4, 4, 6], np.int32)
    tg = np.full((R, NT), -1, np.int32)
    dst = np.full((R, NT), -1, np.int32)
    tg[0, :2], dst[0, :2] = [int(np.argmax(x[0])), 5], [0, 2]
    tg[1, :3], dst[1, :3] = [int(np.argmax(x[1])), 6, 7], [1, 3, 4]
    tg[2, :2], dst[2, :2] = [int(np.argmax(x[2])), 8], [5, -1]
    nt = np.array([2, 3, 2], np.int32)
    D = hip.DeviceBuffer.from_array
    wt, ws = D(np.full(8, 77, U64)), D(np.full(8, 78, U64))
    bufs = [D(a) for a in (x, seq, Ts, ks, Ps, tg, nt, dst)]
    hip.sample_filtered_prob_multi(bufs[0].ptr, R, V, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr,
                                   bufs[6].ptr, bufs[7].ptr, None, None, wt.ptr, ws.ptr)
    wt, ws = wt.download(8, U64), ws.download(8, U64)
    order = [(0, tg[0, 0]), (1, tg[1, 0]), (0, 5), (1, 6), (1, 7), (2, tg[2, 0])]
    ref = _Prob(hip, x[[r for r, _ in order]], seq[[r for r, _ in order]], Ts, ks, Ps,
                np.array([d for _, d in order], np.int32)).launch()
    assert wt[:6].tobytes() == ref["wt"].tobytes() and ws[:6].tobytes() == ref["ws"].tobytes()
    assert ws[0] == ws[2] and ws[1] == ws[3] == ws[4]  # siblings share one total
    assert (wt[6:] == 77).all() and (ws[6:] == 78).all()


# ------------------------------------------------------------ hpa_sample_filtered_exn
class _DrawN(_Draw):
    def launch_n(self, lists, active=None):
        h, R = self.hip, self.R
        ex = np.full((R, NT), -1, np.int32)
        for r, l in enumerate(lists):
            ex[r, :len(l)] = l
        D = h.DeviceBuffer.from_array
        st, nxt = D(self.seeds), D(np.full(R, -5, np.int32))
        nk, cut = D(np.full(R, -9, np.int32)), D(np.full(R, -123.0, np.float32))
        d_ex, d_n = D(ex), D(np.array([len(l) for l in lists], np.int32))
        d_act = D(np.asarray(active, np.int32)) if active is not None else None
        h.sample_filtered_exn(self.xptr, R, self.V, self.T.ptr, self.k.ptr, self.P.ptr, st.ptr, nxt.ptr, None, None,
                              d_act.ptr if d_act else None, nk.ptr, cut.ptr, d_ex.ptr, d_n.ptr)
        return dict(next=nxt.download(R, np.int32), nk=nk.download(R, np.int32), cut=cut.download(R, np.float32),
                    st=st.download(R, U64))


def _exn_case(hip, V, R, seed):
    rng = np.random.default_rng(seed)
    x = _rows(V, R, rng)
    Ts, ks, Ps = _settings(V)
    sel = np.arange(R) % Ts.size
    T, k, P = Ts[sel], ks[sel], Ps[sel]
    seeds = np.arange(R, dtype=U64) * U64(2654435761) + U64(seed + 1)
    return x, T, k, P, seeds, _DrawN(hip, x, T, k, P, seeds), rng


ALL = ("next", "st", "nk", "cut")


@pytest.mark.parametrize("V,R", [(5, 12), (1027, 24), (50257, 12)])
def test_exn_with_at_most_one_id_is_the_existing_sampler_bit_for_bit(hip, V, R):
    x, T, k, P, seeds, dev, rng = _exn_case(hip, V, R, 21 + V)
    plain = dev.launch()
    _same(plain, dev.launch_n([[] for _ in range(R)]), ALL)
    excl = plain["next"].copy()
    excl[::5] = -1
    excl[1::5] = V + 2
    _same(dev.launch(exclude=excl), dev.launch_n([[int(e)] for e in excl]), ALL)


def _kept(x, T, plain, r):
    return sr.kept_indices(x[r], int(plain["nk"][r]), plain["cut"][r]) if T[r] > 0 else np.arange(0)


@pytest.mark.parametrize("V,R", [(5, 12), (1027, 24), (50257, 12)])
def test_exn_lists_draw_from_the_multi_id_residual(hip, V, R):
    x, T, k, P, seeds, dev, rng = _exn_case(hip, V, R, 33 + V)
    plain = dev.launch()
    lists, kept_ties = [], 0
    for r in range(R):
        kept = _kept(x, T, plain, r)
        unkept = np.setdiff1d(np.arange(V), kept)
        m = 2 + r % 6
        ties = np.intersect1d(np.flatnonzero(x[r] == plain["cut"][r]), kept)
        ids = [int(plain["next"][r])]
        if ties.size:
            ids.append(int(ties[-1]))  # a kept tie at the cut
            kept_ties += T[r] > 0 and ties[-1] != plain["next"][r]
        ids += [int(i) for i in rng.permutation(kept)[:2]]
        if unkept.size:
            ids.append(int(unkept[unkept.size // 2]))
        ids += [ids[0], V + r, -3]  # a repeat and ids outside [0, V)
        lists.append([ids[i] for i in rng.permutation(len(ids))][:m])
    out = dev.launch_n(lists)
    _same(out, dev.launch_n(lists), ALL)
    drawn_elsewhere = 0
    for r in range(R):
        s, u = sr.coin(int(seeds[r]))
        assert int(out["st"][r]) == s  # one coin
        n, cut, nxt = int(out["nk"][r]), out["cut"][r], int(out["next"][r])
        assert n == plain["nk"][r] and cut.tobytes() == plain["cut"][r].tobytes()  # the filter, not the removal
        if T[r] == 0:
            assert nxt == int(np.argmax(x[r]))  # greedy rows ignore the list
            continue
        kept = _kept(x, T, plain, r)
        removed = set(lists[r]) & set(kept.tolist())
        if len(removed) == n:
            assert nxt == plain["next"][r]  # removals that would leave nothing are dropped
            continue
        assert nxt in kept and nxt not in removed, (r, nxt, lists[r])
        ts.check_pick_residual_multi(x[r], T[r], n, cut, lists[r], u, nxt, sr.tolerance(x[r], T[r]))
        drawn_elsewhere += nxt != plain["next"][r]
    assert drawn_elsewhere > 0
    if V >= 64:
        assert kept_ties > 0


def test_exn_one_id_left_is_returned_and_a_covered_set_is_the_plain_pick(hip):
    V, R = 1027, 24
    x, T, k, P, seeds, dev, rng = _exn_case(hip, V, R, 77)
    plain = dev.launch()
    one_left, all_gone, survivors = [], [], []
    for r in range(R):
        kept = _kept(x, T, plain, r)
        if T[r] > 0 and 2 <= kept.size <= NT + 1:
            keep = int(kept[r % kept.size])
            one_left.append([int(i) for i in kept if i != keep][:NT])
            survivors.append(keep if kept.size - 1 <= NT else None)
        else:
            one_left.append([])
            survivors.append(None)
        all_gone.append([int(i) for i in kept] if T[r] > 0 and kept.size <= NT else [])
    assert sum(s is not None for s in survivors) >= 4 and sum(bool(l) for l in all_gone) >= 4
    out = dev.launch_n(one_left)
    for r in range(R):
        if survivors[r] is not None:
            assert out["next"][r] == survivors[r], (r, one_left[r])
    _same(plain, dev.launch_n(all_gone), ALL)


def test_exn_inactive_rows_are_untouched(hip):
    V, R = 1027, 12
    x, T, k, P, seeds, dev, rng = _exn_case(hip, V, R, 5)
    plain = dev.launch()
    lists = [[int(plain["next"][r]), 3] for r in range(R)]
    active = np.array([r % 3 != 1 for r in range(R)], np.int32)
    out = dev.launch_n(lists, active=active)
    full = dev.launch_n(lists)
    off = active == 0
    assert (out["next"][off] == -5).all() and (out["nk"][off] == -9).all() and (out["st"][off] == seeds[off]).all()
    for key in ALL:
        assert out[key][~off].tobytes() == full[key][~off].tobytes(), key


# ------------------------------------------------------------ hpa_spec_tree_accept
def _tree_masses(rng, parents, kind):
    """(w_target, w_total) packed by draft: one total per node, its children's
    masses disjoint parts of it"""
    n = len(parents)
    wt, ws = [0] * n, [0] * n
    for node in range(n + 1):
        kids = ts.children(parents, node)
        if not kids:
            continue
        if kind == "greedy":  # temperature 0: (1, 1) for at most one child, (0, 1) for the rest
            hit = int(rng.integers(-1, len(kids)))
            for i, c in enumerate(kids):
                wt[c - 1], ws[c - 1] = int(i == hit), 1
            continue
        S = int(rng.integers(1 << 20, 1 << 62))
        left = S
        for i, c in enumerate(kids):
            if kind == "zero":
                w = 0
            elif kind == "total":  # the last child is all that remains: accepted whenever it is reached
                w = left if i == len(kids) - 1 else int(left * rng.random() * 0.6)
            else:
                w = int(left * rng.choice([0.0, 0.05, 0.5, 0.95]) * rng.random())
            wt[c - 1], ws[c - 1] = w, S
            left -= w
    return wt, ws


@pytest.mark.parametrize("kind", ["generic", "zero", "total", "greedy"])
def test_spec_tree_accept_is_the_integer_walk(hip, kind):
    rng = np.random.default_rng({"generic": 1, "zero": 2, "total": 3, "greedy": 4}[kind])
    shapes = [list(p) for n in range(0, 5) for p in tr.all_parent_arrays(n)]  # 34
    while len(shapes) < 69:
        shapes.append([int(rng.integers(0, j + 1)) for j in range(7)])
    shapes.insert(40, None)  # one len = 0 sequence
    B = len(shapes)
    assert B == 70  # two workgroups
    lens = np.array([0 if p is None else len(p) + 1 for p in shapes], np.int32)
    nd = np.maximum(lens - 1, 0)
    draft0 = (np.cumsum(nd) - nd).astype(np.int32)
    ND = int(nd.sum())
    row0 = (np.cumsum(lens) - lens).astype(np.int32)
    start = rng.integers(0, 500, B).astype(np.int32)
    drafts = rng.integers(0, 50257, ND).astype(np.int32)
    parents = np.concatenate([np.asarray(p, np.int32) for p in shapes if p]).astype(np.int32)
    wt, ws = np.zeros(ND, U64), np.ones(ND, U64)
    for b, p in enumerate(shapes):
        if p:
            a, s = _tree_masses(rng, p, kind)
            wt[draft0[b]:draft0[b] + nd[b]] = np.array(a, U64)
            ws[draft0[b]:draft0[b] + nd[b]] = np.array(s, U64)
    seeds = rng.integers(1, 1 << 63, B, dtype=np.uint64)

    D = hip.DeviceBuffer.from_array
    ins = [D(a) for a in (wt, ws, drafts, parents, draft0, start, row0, lens)]
    d_state, d_pos = D(seeds), D(np.full(B, -3, np.int32))
    d_acc, d_cont, d_nex = (D(np.full(B, 55, np.int32)) for _ in range(3))
    d_path, d_ex = D(np.full((B, tr.MR), 55, np.int32)), D(np.full((B, NT), 55, np.int32))
    hip.spec_tree_accept(*[b.ptr for b in ins], B, d_state.ptr, d_acc.ptr, d_path.ptr, d_cont.ptr, d_ex.ptr, d_nex.ptr,
                         d_pos.ptr)
    acc, cont, nex, pos = (b.download(B, np.int32) for b in (d_acc, d_cont, d_nex, d_pos))
    path = d_path.download(B * tr.MR, np.int32).reshape(B, tr.MR)
    ex = d_ex.download(B * NT, np.int32).reshape(B, NT)
    state = d_state.download(B, U64)
    seen = set()
    for b, p in enumerate(shapes):
        if p is None:
            assert (acc[b], cont[b], nex[b], pos[b]) == (-1, -1, 0, -3) and state[b] == seeds[b]
            assert (ex[b] == -1).all() and (path[b] == 55).all()
            continue
        sl = slice(draft0[b], draft0[b] + nd[b])
        st, want_path, cur, rej, coins, rem = ts.walk(int(seeds[b]), wt[sl], ws[sl], drafts[sl], p)
        a = len(want_path)
        assert (int(acc[b]), int(cont[b]), int(pos[b]), int(nex[b])) == (a, row0[b] + cur, start[b] + a, len(rej)), b
        assert path[b, :a].tolist() == want_path and (path[b, a:] == 55).all(), b
        assert ex[b].tolist() == rej + [-1] * (NT - len(rej)), b
        assert int(state[b]) == st, b
        kids = ts.children(p, cur)
        seen.add("leaf" if not kids else "all rejected" if len(kids) > 1 else "one rejected")
        if a and want_path[0] != ts.children(p, 0)[0]:
            seen.add("non-first sibling")
        if kind == "zero":
            assert a == 0 and len(rej) == len(ts.children(p, 0))
        if kind == "total":
            assert not kids  # some child is always accepted: the walk ends on a leaf
        if kind == "greedy":
            assert len(coins) >= a
    if kind in ("generic", "greedy"):
        assert seen == {"leaf", "all rejected", "one rejected", "non-first sibling"}, seen
