"""The small kernels of a tree pass against tests/tree_ref64.py, exactly:

  hpa_verify_tree_rows    tok / pos / seq / slot / anc of random trees
  hpa_verify_tree_accept  random trees with constructed greedy ids: a match at
                          every depth, a match on a non-first child, no match,
                          len = 0
  hpa_pool_compact_path   a 2-layer, 2-head pool of random bytes, P = 8 and 16:
                          sources and destinations in different pages, a = 0,
                          a path that is consecutive already, an untouched
                          sequence; afterwards the destination slots hold the
                          sources' original bytes and every other byte of the
                          pool is unchanged
"""
import ctypes

import numpy as np
import pytest

import tree_ref64 as tr

pytestmark = pytest.mark.gpu

MR = tr.MR
_I = ctypes.POINTER(ctypes.c_int)
_U8 = ctypes.POINTER(ctypes.c_ubyte)


def _p(buf, t=_I):
    return ctypes.cast(buf.ptr, t)


def _random_tree(rng, nd):
    return [int(rng.integers(0, j + 1)) for j in range(nd)]


def _batch(rng, B):
    """B sequences: n_draft in 0..7 with every value present, two of them skipped (len 0)"""
    nds = list(range(8)) + [int(rng.integers(0, 8)) for _ in range(B - 8)]
    rng.shuffle(nds)
    lens = np.array([n + 1 for n in nds], np.int32)
    lens[[3, B - 2]] = 0
    trees = [_random_tree(rng, max(n - 1, 0)) for n in lens]
    ids = [rng.integers(0, 50, len(t)).astype(np.int32) for t in trees]
    start = rng.integers(0, 900, B).astype(np.int32)
    nxt = rng.integers(0, 50, B).astype(np.int32)
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    d0 = np.concatenate([[0], np.cumsum([len(t) for t in trees])[:-1]]).astype(np.int32)
    return lens, trees, ids, start, nxt, row0, d0


def _upload(hip, lens, trees, ids, start, nxt, row0, d0):
    flat = lambda xs: np.concatenate([np.asarray(x, np.int32) for x in xs] + [np.zeros(1, np.int32)])  # noqa: E731
    return dict(next=hip.DeviceBuffer.from_array(nxt), drafts=hip.DeviceBuffer.from_array(flat(ids)),
                parents=hip.DeviceBuffer.from_array(flat(trees)), d0=hip.DeviceBuffer.from_array(d0),
                start=hip.DeviceBuffer.from_array(start), row0=hip.DeviceBuffer.from_array(row0),
                len=hip.DeviceBuffer.from_array(lens))


def test_tree_rows_match_the_restatement(hip):
    rng = np.random.default_rng(3)
    B = 24
    lens, trees, ids, start, nxt, row0, d0 = _batch(rng, B)
    R = int(lens.sum())
    d = _upload(hip, lens, trees, ids, start, nxt, row0, d0)
    out = {k: hip.DeviceBuffer.from_array(np.full(R + 4, -7, np.int32)) for k in ("tok", "pos", "seq", "slot")}
    anc = hip.DeviceBuffer.from_array(np.full(R + 4, 0xEE, np.uint8))
    L = hip.lib()
    hip.check(L.hpa_verify_tree_rows(_p(d["next"]), _p(d["drafts"]), _p(d["parents"]), _p(d["d0"]), _p(d["start"]),
                                     _p(d["row0"]), _p(d["len"]), B, _p(out["tok"]), _p(out["pos"]), _p(out["seq"]),
                                     _p(out["slot"]), _p(anc, _U8)), "tree rows")
    hip.check(L.hpa_synchronize())
    got = {k: v.download(R + 4, np.int32) for k, v in out.items()}
    got_anc = anc.download(R + 4, np.uint8)
    for b in range(B):
        if lens[b] == 0:
            continue
        tok, pos, slot, m = tr.rows(nxt[b], ids[b], trees[b], start[b])
        r = slice(row0[b], row0[b] + lens[b])
        assert np.array_equal(got["tok"][r], tok) and np.array_equal(got["pos"][r], pos), b
        assert np.array_equal(got["slot"][r], slot) and (got["seq"][r] == b).all(), b
        assert np.array_equal(got_anc[r], m), (b, trees[b])
    for k in got:  # nothing past the rows
        assert (got[k][R:] == -7).all()
    assert (got_anc[R:] == 0xEE).all()


def _tops(rng, nxt_tok, ids, par, kind):
    """greedy ids per node that make the walk end where `kind` says; returns (top, wanted path)"""
    n = len(ids) + 1
    tok = [int(nxt_tok)] + [int(t) for t in ids]
    top = [1000 + i for i in range(n)]  # matches no token (tokens < 50)
    kids = lambda c: [j + 1 for j in range(n - 1) if par[j] == c]  # noqa: E731
    path = []
    if kind == "none" or n == 1:
        return top, path
    cur = 0
    while kids(cur):
        ks = kids(cur)
        c = ks[-1] if kind == "last_child" else ks[0] if kind == "first_child" else ks[int(rng.integers(0, len(ks)))]
        top[cur] = tok[c]
        path.append(c)
        cur = c
        if kind == "one" or (kind == "random" and rng.integers(0, 3) == 0):
            break
    return top, path


@pytest.mark.parametrize("kind", ["first_child", "last_child", "random", "one", "none"])
def test_tree_accept_matches_the_walk(hip, kind):
    """trees whose siblings carry distinct tokens (as the engine requires); the
    greedy ids lead down the first children to a leaf, down the last children
    (a non-first child wherever a node has two), down a random branch to a
    random depth, one step, or nowhere"""
    rng = np.random.default_rng([5, len(kind)])
    B = 70  # more than one 64-thread block
    lens, trees, ids, start, nxt, row0, d0 = _batch(rng, B)
    trees[int(np.flatnonzero(lens == 8)[0])] = list(tr.CHAIN)  # one chain: a match at every depth down to 7
    ids = [np.arange(len(t), dtype=np.int32) + 1 for t in trees]  # distinct tokens per sequence, none equal to next = 0
    nxt[:] = 0
    R = int(lens.sum())
    top = np.full(R + 1, -3, np.int32)
    tokr = np.full(R + 1, -4, np.int32)
    want = []
    for b in range(B):
        if lens[b] == 0:
            want.append(None)
            continue
        t, path = _tops(rng, nxt[b], ids[b], trees[b], kind)
        top[row0[b]:row0[b] + lens[b]] = t
        tokr[row0[b]:row0[b] + lens[b]] = [nxt[b]] + ids[b].tolist()
        assert tr.accept(tokr[row0[b]:row0[b] + lens[b]], t, trees[b]) == path
        want.append(path)
    if kind == "last_child":  # walks that step onto a node with an older sibling
        assert sum(1 for b in range(B) if want[b] and any(trees[b][c - 1] in trees[b][:c - 1] for c in want[b])) >= 10
    d = _upload(hip, lens, trees, ids, start, nxt, row0, d0)
    d_tok, d_top = hip.DeviceBuffer.from_array(tokr), hip.DeviceBuffer.from_array(top)
    acc = hip.DeviceBuffer.from_array(np.full(B, -9, np.int32))
    path = hip.DeviceBuffer.from_array(np.full(B * MR, -9, np.int32))
    cont = hip.DeviceBuffer.from_array(np.full(B, -9, np.int32))
    pos0 = rng.integers(0, 5, B).astype(np.int32) - 100
    pos = hip.DeviceBuffer.from_array(pos0)
    L = hip.lib()
    hip.check(L.hpa_verify_tree_accept(_p(d_tok), _p(d_top), _p(d["parents"]), _p(d["d0"]), _p(d["start"]),
                                       _p(d["row0"]), _p(d["len"]), B, _p(acc), _p(path), _p(cont), _p(pos)),
              "tree accept")
    hip.check(L.hpa_synchronize())
    g_acc, g_path = acc.download(B, np.int32), path.download((B, MR), np.int32)
    g_cont, g_pos = cont.download(B, np.int32), pos.download(B, np.int32)
    for b in range(B):
        if want[b] is None:
            assert g_acc[b] == -1 and g_cont[b] == -1 and g_pos[b] == pos0[b] and (g_path[b] == -9).all(), b
            continue
        a = len(want[b])
        assert g_acc[b] == a and g_path[b, :a].tolist() == want[b] and (g_path[b, a:] == -9).all(), (b, want[b])
        assert g_cont[b] == row0[b] + (want[b][-1] if a else 0) and g_pos[b] == start[b] + a, b
    depths = sorted({len(w) for w in want if w is not None})
    print(f"TREEACCEPT {kind}: accepted depths {depths}")
    if kind in ("first_child", "last_child"):
        assert depths[-1] == 7 and len(depths) >= 4


@pytest.mark.parametrize("P", [8, 16])
def test_compact_path_moves_exactly_the_path(hip, P):
    NL, NH, HS = 2, 2, 64
    rng = np.random.default_rng([9, P])
    # (start, path): slots start + path[k-1] -> start + k
    cases = [(P - 3, [3, 5, 7]),          # sources in the next page, destinations span the edge
             (2 * P - 2, [2, 4]),         # destination 1 is a page's last slot, its source the next page's first
             (5, []),                     # a = 0
             (P + 1, [1, 2, 3]),          # consecutive already: nothing moves
             (3, None),                   # untouched (n_accepted = -1)
             (P - 3, [1, 4, 5, 6, 7]),    # first in place, then a gap across the edge
             (P - 2, [7]),                # the last node into slot 1, from the next page
             (3 * P - 8, [1, 2, 3, 4, 5, 6, 7])]
    B = len(cases)
    pages_per = 5
    pool = hip.Pool(NL, NH, P, B * pages_per + 2)
    nfl = pool.s.bytes // 4
    host = rng.integers(0, 2 ** 32, nfl, dtype=np.uint32)  # any bytes: the copy is bitwise
    L = hip.lib()
    hip.check(L.hpa_memcpy(pool.s.base, host.ctypes.data, host.nbytes), "pool upload")
    perm = rng.permutation(B * pages_per + 2).astype(np.int32)
    bt = perm[:B * pages_per].reshape(B, pages_per).copy()
    start = np.array([c[0] for c in cases], np.int32)
    acc = np.array([-1 if c[1] is None else len(c[1]) for c in cases], np.int32)
    path = np.full((B, MR), 99, np.int32)  # entries past a are never read
    for b, c in enumerate(cases):
        if c[1]:
            path[b, :len(c[1])] = c[1]
    d_bt, d_start = hip.DeviceBuffer.from_array(bt), hip.DeviceBuffer.from_array(start)
    d_path, d_acc = hip.DeviceBuffer.from_array(path), hip.DeviceBuffer.from_array(acc)

    def k_index(layer, page, head, slot, dim):
        return L.hpa_pool_k_index(pool.ref, layer, int(page), head, slot, dim)

    def v_index(layer, page, head, slot, dim):
        return L.hpa_pool_v_index(pool.ref, layer, int(page), head, slot, dim)

    want = host.copy()
    moved = 0
    for b, (st, pth) in enumerate(cases):
        for k, p in enumerate(pth or [], 1):
            if p == k:
                continue
            s, t = st + p, st + k
            for layer in range(NL):
                for head in range(NH):
                    for dim in range(HS):
                        for index in (k_index, v_index):
                            want[index(layer, bt[b, t // P], head, t % P, dim)] = \
                                host[index(layer, bt[b, s // P], head, s % P, dim)]
                            moved += 1
            if s // P != t // P:
                cases[b] = (st, pth, True)
    assert sum(1 for c in cases if len(c) == 3) >= 4  # sources and destinations in different pages
    assert moved == (3 + 2 + 4 + 1) * NL * NH * HS * 2 and not np.array_equal(want, host)
    hip.check(L.hpa_pool_compact_path(pool.ref, _p(d_bt), pages_per, _p(d_start), _p(d_path), _p(d_acc), B),
              "compact_path")
    hip.check(L.hpa_synchronize())
    got = np.empty_like(host)
    hip.check(L.hpa_memcpy(got.ctypes.data, pool.s.base, got.nbytes), "pool download")
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, f"{diff.size} words differ, first at {diff[:4]}"


def test_compact_path_refuses_other_pools(hip):
    """a bf16 pool: nonzero, nothing launched (the pool keeps its bytes)"""
    pool = hip.Pool(1, 2, 16, 4, dtype=hip.HPA_BF16)
    L = hip.lib()
    hip.check(L.hpa_memset_async(pool.s.base, 0x5A, pool.s.bytes))
    bt = hip.DeviceBuffer.from_array(np.arange(4, dtype=np.int32))
    start = hip.DeviceBuffer.from_array(np.array([2], np.int32))
    path = hip.DeviceBuffer.from_array(np.array([3, 5, 0, 0, 0, 0, 0, 0], np.int32))
    acc = hip.DeviceBuffer.from_array(np.array([2], np.int32))
    assert L.hpa_pool_compact_path(pool.ref, _p(bt), 4, _p(start), _p(path), _p(acc), 1) != 0
    hip.check(L.hpa_synchronize())
    got = np.empty(pool.s.bytes, np.uint8)
    hip.check(L.hpa_memcpy(got.ctypes.data, pool.s.base, got.nbytes))
    assert (got == 0x5A).all()
