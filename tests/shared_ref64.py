"""Shared-prefix decode attention restated in numpy: the plan
(gpt2_attn_shared_plan), the cascade the two launches compute, and the case
set that aims a peaked softmax at the cascade's edges.  Numpy only.

plan(bt, pos, P, min_tiles, min_members): the algorithm paged_infer.h states,
written from that text -- common(a, b) leading equal pages, share in whole
64-token tiles, leaders in index order, candidates by share descending then
index ascending, the k <= 7 with the largest k * t_k (the larger k on a tie).

attend_cascade(q, K, V, ctx, tiles, splits): one query in the kernels' form,
float64 like attn_ref64.attend_online: the prefix tiles [0, tiles) dealt over
`splits` ranges (range s: tiles s * tiles // splits .. (s + 1) * tiles //
splits), each folded from m = -10000 into an unnormalised (m, l, acc) record
(a range without a tile: the neutral record m = -10000, l = 0, acc = 0); the
suffix tiles from `tiles` on folded the same way; then the merge M = max of
every m, l and acc rescaled by exp(m - M), records in split order ahead of the
suffix, out = acc / l (0 where l == 0).  MUTATIONS are the ways the cascade
could be subtly wrong.

shared_cases(P): one batch, one decode row per sequence.  A group is one
prefix (K, V of whole 64-token tiles) held in shared pages; a member continues
it with its own suffix from own_from[row] on.  Units (the device tables) are
written down by hand, not planned:
    t = 1 unit of 2, t = 2 unit of 3, t = 5 unit of 8 (uniform K, V; hot and
    pair keys at 0, 64t - 1, 64t, pos and the prefix split edges of 2 and 3
    ranges); 9 sharers of one t = 2 prefix as a unit of 8 and a unit of 1 over
    the same pages; a unit of 3 at t = 2 two of whose members share 5 tiles;
    ramps of 300 nats in both directions across the boundary (t = 2 and 5);
    the single above-floor key in the prefix only / in the suffix only / nowhere
    (output exactly 0); five sequences in no unit (ctx 1 .. 200).
Member positions: 64t, 64t + 63, 64t + 64 and 64t + 300 among them.  Rows are
permuted so that non-members sit between the members of a unit by index.
"""
import numpy as np

import attn_ref64 as ar

HS, NH, C = ar.HS, ar.NH, ar.C
MAX_ROWS = 8
SPLITS = (1, 2, 3)


# ---------------------------------------------------------------- the plan
def common_pages(bt, a, b):
    n = 0
    while n < bt.shape[1] and bt[a, n] >= 0 and bt[a, n] == bt[b, n]:
        n += 1
    return n


def share(bt, pos, P, a, b):
    return min(common_pages(bt, a, b) * P, int(pos[a]), int(pos[b])) // 64


def plan(bt, pos, P, min_tiles=1, min_members=2):
    """-> (units [(members, tiles)], seq_skip [B])"""
    bt = np.asarray(bt)
    B = bt.shape[0]
    unassigned = [b for b in range(B) if pos[b] >= 64]
    units, skip = [], np.zeros(B, np.int32)
    while unassigned:
        a = unassigned[0]
        cand = [(share(bt, pos, P, a, b), b) for b in unassigned[1:]]
        cand = sorted([c for c in cand if c[0] >= min_tiles], key=lambda c: (-c[0], c[1]))[:MAX_ROWS - 1]
        best_k, best = 0, -1
        for k in range(1, len(cand) + 1):
            if k * cand[k - 1][0] >= best:
                best_k, best = k, k * cand[k - 1][0]
        if best_k and best_k + 1 >= min_members:
            members = [a] + [b for _, b in cand[:best_k]]
            t = cand[best_k - 1][0]
            units.append((members, t))
            skip[members] = t
            unassigned = [b for b in unassigned if b not in members]
        else:
            unassigned = unassigned[1:]
    return units, skip


def plan_tables(units, skip, max_units):
    """the C tables of a plan: unit_members [max_units][8] -1 padded, unit_tiles [max_units]"""
    members = np.full((max_units, MAX_ROWS), -1, np.int32)
    tiles = np.zeros(max_units, np.int32)
    for u, (m, t) in enumerate(units):
        members[u, :len(m)] = m
        tiles[u] = t
    return members, tiles, np.asarray(skip, np.int32)


def check_invariants(bt, pos, P, units):
    """what the kernels rely on; raises AssertionError"""
    seen = set()
    for members, t in units:
        assert 2 <= len(members) <= MAX_ROWS and t >= 1
        assert not (seen & set(members)), "a sequence in two units"
        seen |= set(members)
        npages = (64 * t + P - 1) // P
        for m in members:
            assert 64 * t <= pos[m]
            assert (bt[m, :npages] >= 0).all() and np.array_equal(bt[m, :npages], bt[members[0], :npages])


# ---------------------------------------------------------------- the cascade
MUTATIONS = ("drop_prefix", "prefix_short_one_tile", "merge_no_rescale", "other_members_q", "neutral_m_zero")


def _partial(q, K, V, t_lo, t_hi, ctx, neutral_m=ar.FLOOR):
    """tiles [t_lo, t_hi) of keys < ctx folded from the floor: (m, l, acc), unnormalised"""
    if t_hi <= t_lo:
        return neutral_m, 0.0, np.zeros(HS)
    m_run, l, acc = ar.FLOOR, 0.0, np.zeros(HS)
    for it in range(t_lo, t_hi):
        idx = np.arange(64 * it, min(64 * it + 64, ctx))
        if not idx.size:
            continue
        s = K[idx] @ q / 8.0
        mn = max(m_run, s.max())
        alpha = np.exp(m_run - mn)
        d = s - mn
        p = np.where(d >= -100.0, np.exp(np.maximum(d, -100.0)), 0.0)
        l = l * alpha + p.sum()
        acc = acc * alpha + p @ V[idx]
        m_run = mn
    return m_run, l, acc


def attend_cascade(q, K, V, ctx, tiles, splits, mutate=None, q_other=None):
    """one query, float64.  tiles: the prefix tiles its unit streams (0: none,
    no record read); q_other: another member's query (mutation other_members_q)"""
    q = np.asarray(q, np.float64)
    K = np.asarray(K, np.float64)
    V = np.asarray(V, np.float64)
    parts = []
    if tiles > 0 and mutate != "drop_prefix":
        t_pre = tiles - 1 if mutate == "prefix_short_one_tile" else tiles
        qp = np.asarray(q_other, np.float64) if mutate == "other_members_q" and q_other is not None else q
        for s in range(splits):
            parts.append(_partial(qp, K, V, s * t_pre // splits, (s + 1) * t_pre // splits, 64 * t_pre,
                                  neutral_m=0.0 if mutate == "neutral_m_zero" else ar.FLOOR))
    parts.append(_partial(q, K, V, tiles, (ctx + 63) // 64, ctx))
    M = max(p[0] for p in parts)
    l, acc = 0.0, np.zeros(HS)
    for m, pl, pa in parts:  # records in split order, the suffix last
        f = 1.0 if mutate == "merge_no_rescale" else np.exp(max(m - M, -745.0))
        l += pl * f
        acc = acc + pa * f
    return acc / l if l != 0.0 else np.zeros(HS)


# ---------------------------------------------------------------- the case set
class SharedCases:
    """cs: attn_ref64.Cases with one sequence per row (row i <-> cs.seqs[i]);
    group[i]: the row's prefix group (-1: none); own_from[i]: the first token
    of row i that lies in its own pages (a multiple of 64; 0 without a group):
    rows a, b of one group hold the same pages for tokens below
    min(own_from[a], own_from[b]).  units: [(member rows, tiles)]."""

    def __init__(self, cs, group, own_from, units):
        self.cs, self.group, self.own_from, self.units = cs, np.array(group), np.array(own_from), units
        self.B = len(cs.seq)
        self.pos = cs.ctx - 1
        self.skip = np.zeros(self.B, np.int32)
        self.unit_of = np.full(self.B, -1, np.int32)
        for u, (m, t) in enumerate(units):
            self.skip[m] = t
            self.unit_of[m] = u

    def tables(self, max_units=None):
        mu = max(self.B // 2, len(self.units)) if max_units is None else max_units
        return plan_tables(self.units, self.skip, mu)


def _aim_positions(t, pos):
    p = [0, 64 * t - 1, 64 * t, pos]
    for S in SPLITS[1:]:
        for s in range(1, S):
            e = 64 * (s * t // S)
            p += [e - 1, e]
    return sorted({min(max(int(j), 0), pos) for j in p})


def shared_cases(P, seed=0):
    rng = np.random.default_rng([seed, P, 77])
    rows = []   # dicts: K, V (ctx, C), q (C,), kinds, group, own_from
    units = []  # (row indices into `rows`, tiles)

    def uniform_group(g, t_pages, t_unit, members, n_rot):
        """members: [(own_from_tiles, pos)]; K, V uniform; kinds rotate hot / pair / uniform"""
        Kp, Vp = rng.uniform(-1, 1, (64 * t_pages, C)), rng.uniform(-1, 1, (64 * t_pages, C))
        out = []
        for i, (own_t, pos) in enumerate(members):
            ctx = pos + 1
            K = np.concatenate([Kp[:64 * own_t], rng.uniform(-1, 1, (ctx - 64 * own_t, C))]).astype(np.float32)
            V = np.concatenate([Vp[:64 * own_t], rng.uniform(-1, 1, (ctx - 64 * own_t, C))]).astype(np.float32)
            kind = ("hot", "pair", "hot", "pair", "uniform")[(i + n_rot) % 5]
            aims = _aim_positions(t_unit, pos)
            if kind == "uniform":
                q = rng.uniform(-2, 2, C)
            else:
                q = np.zeros(C, np.float32)
                for h in range(NH):
                    c = slice(h * HS, (h + 1) * HS)
                    j = aims[(NH * i + h + n_rot) % len(aims)]
                    if kind == "pair":
                        j = min(j, pos - 1)
                    q[c] = ar._aimed(K[:, c], K[j, c] + K[j + 1, c] if kind == "pair" else K[j, c])
            out.append(len(rows))
            rows.append(dict(K=K, V=V, q=q, kinds=[kind] * NH, group=g, own_from=64 * own_t))
        return out

    g = 0
    # t = 1, unit of 2; t = 2, unit of 3; t = 5, unit of 8
    r = uniform_group(g, 1, 1, [(1, 64), (1, 64 + 63)], 0); units.append((r, 1)); g += 1
    r = uniform_group(g, 2, 2, [(2, 128 + 64), (2, 128 + 300), (2, 128 + 5)], 1); units.append((r, 2)); g += 1
    r = uniform_group(g, 5, 5, [(5, 320 + o) for o in (0, 63, 64, 300, 1, 17, 130, 200)], 2); units.append((r, 5)); g += 1
    # 9 sharers of one prefix: a unit of 8 and a unit of 1 over the same pages
    r = uniform_group(g, 2, 2, [(2, 128 + o) for o in (0, 63, 64, 300, 7, 8, 9, 33, 100)], 3)
    units.append((r[:8], 2)); units.append((r[8:], 2)); g += 1
    # two members share 5 tiles between themselves, the unit streams 2
    r = uniform_group(g, 5, 2, [(5, 320 + 10), (5, 320 + 64), (2, 128 + 20)], 4); units.append((r, 2)); g += 1
    # ramps across the boundary: (up, down) at t = 2, (down, up) at t = 5; members differ in V past the prefix
    for t, ups, off in ((2, (True, False), 37), (5, (False, True), 300)):
        ctx = 64 * t + off + 1
        kq = [ar._ramp_keys(rng, ctx, up) for up in ups]
        K = np.concatenate([k for k, _ in kq], 1).astype(np.float32)
        q = np.concatenate([qq for _, qq in kq])
        Vp = rng.uniform(-1, 1, (64 * t, C))
        r = []
        for _ in range(2):
            V = np.concatenate([Vp, rng.uniform(-1, 1, (ctx - 64 * t, C))]).astype(np.float32)
            r.append(len(rows))
            rows.append(dict(K=K, V=V, q=q, kinds=["ramp_up" if up else "ramp_down" for up in ups], group=g,
                             own_from=64 * t))
        units.append((r, t)); g += 1
    # the floor: the one key in the prefix only (t = 2: at 64t - 1 for head 0, at 0 for head 1) ...
    t = 2
    offs = (0, 64, 300)
    ctx_max = 64 * t + max(offs) + 1
    kq = [ar._floor_keys(rng, ctx_max, one) for one in (64 * t - 1, 0)]
    K = np.concatenate([k for k, _ in kq], 1).astype(np.float32)
    q = np.concatenate([qq for _, qq in kq])
    Vp = rng.uniform(-1, 1, (64 * t, C))
    r = []
    for off in offs:
        ctx = 64 * t + off + 1
        V = np.concatenate([Vp, rng.uniform(-1, 1, (ctx - 64 * t, C))]).astype(np.float32)
        r.append(len(rows))
        rows.append(dict(K=K[:ctx], V=V, q=q, kinds=["below_floor_one"] * NH, group=g, own_from=64 * t))
    units.append((r, t)); g += 1
    # ... in the suffix only (at pos / at 64t), and nowhere: exactly 0
    t = 1
    kq = [ar._floor_keys(rng, 64 * t + 301, None) for _ in range(NH)]
    Kall = np.concatenate([k for k, _ in kq], 1).astype(np.float32)
    us = [qq.astype(np.float64) / -20100.0 for _, qq in kq]
    q = np.concatenate([qq for _, qq in kq])
    Vp = rng.uniform(-1, 1, (64 * t, C))
    r = []
    for off, one in ((63, "pos"), (64, None), (300, "first")):
        ctx = 64 * t + off + 1
        K = Kall[:ctx].copy()
        if one is not None:
            j = ctx - 1 if one == "pos" else 64 * t
            for h in range(NH):
                K[j, h * HS:(h + 1) * HS] = 4.0 * us[h]
        V = np.concatenate([Vp, rng.uniform(-1, 1, (ctx - 64 * t, C))]).astype(np.float32)
        r.append(len(rows))
        rows.append(dict(K=K, V=V, q=q, kinds=["below_floor_all" if one is None else "below_floor_one"] * NH, group=g,
                         own_from=64 * t))
    units.append((r, t)); g += 1
    # sequences in no unit
    for i, ctx in enumerate((1, 63, 64, 65, 200)):
        K = rng.uniform(-1, 1, (ctx, C)).astype(np.float32)
        V = rng.uniform(-1, 1, (ctx, C)).astype(np.float32)
        if i % 2:
            q, kind = rng.uniform(-2, 2, C), "uniform"
        else:
            q = np.concatenate([ar._aimed(K[:, h * HS:(h + 1) * HS], K[(ctx - 1) * h, h * HS:(h + 1) * HS])
                                for h in range(NH)])
            kind = "hot"
        rows.append(dict(K=K, V=V, q=q, kinds=[kind] * NH, group=-1, own_from=0))

    # non-members between members by index: a fixed permutation of the rows
    perm = np.random.default_rng([seed, 5]).permutation(len(rows))
    where = np.empty(len(rows), np.int64)
    where[perm] = np.arange(len(rows))  # old row -> new row
    cs = ar.Cases()
    group, own_from = [], []
    for new in range(len(rows)):
        d = rows[perm[new]]
        cs.seqs.append((d["K"], d["V"]))
        cs.add_row(new, d["K"].shape[0], d["q"], d["kinds"])
        group.append(d["group"])
        own_from.append(d["own_from"])
    units = [([int(where[i]) for i in m], t) for m, t in units]
    return SharedCases(cs.finish(), group, own_from, units)


def cascade_outputs(sc, splits, mutate=None):
    """attend_cascade over every row of sc -> (B, C)"""
    cs = sc.cs
    got = np.zeros((sc.B, C))
    for i in range(sc.B):
        K, V = cs.seqs[i]
        other = None
        if sc.unit_of[i] >= 0:
            m = sc.units[sc.unit_of[i]][0]
            other = cs.q[m[(m.index(i) + 1) % len(m)]]
        for h in range(NH):
            c = slice(h * HS, (h + 1) * HS)
            got[i, c] = attend_cascade(cs.q[i, c], K[:, c], V[:, c], int(cs.ctx[i]), int(sc.skip[i]), splits, mutate,
                                       None if other is None else other[c])
    return got
