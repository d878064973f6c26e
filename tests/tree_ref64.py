"""Tree speculation restated in numpy: node tables (depth, slot, ancestor
mask), the accept walk, the K/V compaction and the n-gram tree drafter.

A tree of n_draft drafts has n = n_draft + 1 nodes: node 0 is the pending
token, draft j (0-based) is node j + 1 and hangs from node parents[j] in
[0, j], so a parent's index is always smaller than its child's.
"""
import itertools

import numpy as np

MR = 8  # HPA_VERIFY_MAX_ROWS


def valid(parents, ids=None):
    """parents[j] in [0, j]; with ids: no two siblings with the same token"""
    for j, p in enumerate(parents):
        if not 0 <= p <= j:
            return False
    if ids is not None:
        seen = set()
        for p, t in zip(parents, ids):
            if (p, t) in seen:
                return False
            seen.add((p, t))
    return True


def depths(parents):
    """depth of every node (n_draft + 1,): 0 for the root"""
    d = [0]
    for p in parents:
        d.append(d[p] + 1)
    return np.array(d, np.int32)


def anc_masks(parents):
    """(n_draft + 1,) uint8: bit i of entry r set iff node i is r or an ancestor of r"""
    m = [1]
    for j, p in enumerate(parents):
        m.append(m[p] | (1 << (j + 1)))
    return np.array(m, np.uint8)


def visible(parents):
    """(n, n) bool: visible[r][i] = node r sees node i's key"""
    m = anc_masks(parents)
    n = len(m)
    return np.array([[bool((int(m[r]) >> i) & 1) for i in range(n)] for r in range(n)])


def rows(pending, ids, parents, start):
    """the row tables of one sequence: tok, pos, slot, anc per node"""
    d = depths(parents)
    n = len(d)
    return (np.array([pending] + list(ids), np.int32), (start + d).astype(np.int32),
            (start + np.arange(n)).astype(np.int32), anc_masks(parents))


def accept(tok, top, parents):
    """the walk: from node 0 to the lowest-indexed child whose token is the
    greedy id of the node it hangs from, while there is one.  Returns the
    path (node indices)"""
    n = len(tok)
    cur, path = 0, []
    while True:
        nxt = [c for c in range(cur + 1, n) if parents[c - 1] == cur and tok[c] == top[cur]]
        if not nxt:
            return path
        cur = nxt[0]
        path.append(cur)


def paths(parents):
    """every root-to-node path of the tree (the empty one included)"""
    out = [[]]
    for j in range(len(parents)):
        p, node = [], j + 1
        while node:
            p.append(node)
            node = parents[node - 1]
        out.append(p[::-1])
    return out


def all_parent_arrays(n_draft):
    return itertools.product(*[range(j + 1) for j in range(n_draft)])


def compact_gather(slots, path):
    """out of place: slot k <- the original slot path[k - 1], the rest unchanged"""
    out = slots.copy()
    for k, p in enumerate(path, 1):
        out[k] = slots[p]
    return out


def compact_in_place(slots, path, descending=False):
    """what the kernel does per lane: k ascending, reading the live array.
    descending: the mutant (wrong whenever a destination is a later source)"""
    out = slots.copy()
    ks = range(len(path), 0, -1) if descending else range(1, len(path) + 1)
    for k in ks:
        if path[k - 1] != k:
            out[k] = out[path[k - 1]]
    return out


def ngram_tree_ref(h, max_ngram, min_ngram, max_nodes, depth, max_branches):
    """gpt2_ngram_draft_tree restated: (ids, parents)"""
    h = list(h)
    n = len(h)
    ids, par = [], []
    if min_ngram < 1 or depth < 1 or max_branches < 1 or not 1 <= max_nodes <= MR - 1:
        return ids, par
    branches = 0
    for g in range(max_ngram, min_ngram - 1, -1):
        for s in range(n - g - 1, -1, -1):
            if h[s:s + g] != h[n - g:]:
                continue
            cur, added = 0, False
            for t in h[s + g:s + g + depth]:
                kids = [j + 1 for j in range(len(ids)) if par[j] == cur and ids[j] == t]
                if kids:
                    cur = kids[0]
                    continue
                if len(ids) == max_nodes:
                    break
                ids.append(t)
                par.append(cur)
                cur = len(ids)
                added = True
            branches += added
            if len(ids) == max_nodes or branches == max_branches:
                return ids, par
    return ids, par


def first_child_chain(ids, parents):
    """the tokens along the first-child chain from the root"""
    out, cur = [], 0
    while True:
        kids = [j for j in range(len(ids)) if parents[j] == cur]
        if not kids:
            return out
        out.append(ids[kids[0]])
        cur = kids[0] + 1


# ---------------------------------------------------------------- tree shapes of the GPU tests (7 drafts)
STAR = [0, 0, 0, 0, 0, 0, 0]
TWO_CHAINS = [0, 1, 2, 0, 4, 5]   # nodes 1-2-3 and 4-5-6 off the root (6 drafts)
BINARY = [0, 0, 1, 1, 2, 2, 3]
CHAIN = [0, 1, 2, 3, 4, 5, 6]
SHAPES = {"star": STAR, "two_chains": TWO_CHAINS, "binary": BINARY, "chain": CHAIN}
