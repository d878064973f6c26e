"""Sampled tree speculation restated in Python integers and exact fractions
(the rule of gpt2_decode_verify_tree_sampled, include/paged_infer.h).

A tree in tree_ref64's layout: node 0 the pending id, draft j = node j + 1
under parents[j] in [0, j], siblings with distinct tokens.  Masses are packed by
draft: w_target[j] the fixed-point mass of draft j's token at its parent's row,
w_total[j] that row's kept total (the same for all children of one node).

  walk            hpa_spec_tree_accept: children in ascending node index, one
                  coin each, accepted iff w * 2^24 > rem * j, rem losing every
                  rejected child's mass
  residual_multi  spec_ref64.residual for a list of removed ids
  dense_tables    gpt2_tree_dense_tables
  first_law /     the law of the emitted tokens with the coins integrated out
  emitted_law     (u uniform on [0, 1): a child is accepted with probability
                  w / rem), in exact fractions
"""
from fractions import Fraction

import numpy as np

import sample_ref64 as sr
import spec_ref64 as sp

NT = 7  # HPA_VERIFY_MAX_ROWS - 1


def accepts(w, rem, j):
    """the integer test: u = j / 2^24 < w / rem"""
    return int(w) * (1 << 24) > int(rem) * int(j)


def clamp_parent(p, j):
    return min(max(int(p), 0), j)


def children(parents, node):
    """the children of `node`, ascending (parents clamped like the device tables)"""
    return [j + 1 for j in range(len(parents)) if clamp_parent(parents[j], j) == node]


def walk(state, w_target, w_total, drafts, parents):
    """One sequence's walk.  Returns (new state, path, final node, the rejected
    children's tokens at the final node in child order, the coins j drawn,
    what is left of the final node's total (None at a leaf))."""
    cur, path, coins = 0, [], []
    while True:
        rej, rem, nxt = [], None, None
        for c in children(parents, cur):
            if rem is None:
                rem = int(w_total[c - 1])
            state, r = sr.xorshift_u32(state)
            j = r >> 8
            coins.append(j)
            w = int(w_target[c - 1])
            if accepts(w, rem, j):
                nxt = c
                break
            rem -= min(w, rem)
            rej.append(int(drafts[c - 1]))
        if nxt is None:
            return state, path, cur, rej, coins, rem
        path.append(nxt)
        cur = nxt


def residual_multi(x, T, kept, ds):
    """(ids, cdf): the kept set without the ids of ds, ascending, and the
    float64 cdf of its renormalised masses.  Ids outside the kept set and
    repeats remove nothing; removals that would leave nothing are all dropped."""
    kept = np.asarray(kept)
    rest = kept[~np.isin(kept, np.asarray(list(ds), np.int64))] if len(ds) else kept
    if rest.size == 0:
        rest = kept
    m = sp.masses(x, kept, T)[np.isin(kept, rest)]
    return rest, np.cumsum(m) / m.sum()


def check_pick_residual_multi(x, T, n, cut, ds, u, nxt, tol):
    """sample_ref64.check_pick on the multi-id residual cdf"""
    kept = sr.kept_indices(x, n, cut)
    assert kept.size == n, (kept.size, n)
    rest, c = residual_multi(x, T, kept, ds)
    at = int(np.searchsorted(rest, nxt))
    assert at < rest.size and rest[at] == nxt, ("pick outside the residual set", nxt, list(ds), n, cut)
    lo = c[at - 1] if at > 0 else 0.0
    assert lo - tol <= float(u) < c[at] + tol, (nxt, list(ds), lo, float(u), c[at], tol)


def dense_tables(trees, row0):
    """gpt2_tree_dense_tables: trees[b] = None | (ids, parents).  Returns lists
    (rows, seq, targets, n_targets, dst), targets / dst padded to NT with -1"""
    rows, seq, tg, nt, dst = [], [], [], [], []
    nd = 0
    for b, t in enumerate(trees):
        if t is None or not len(t[0]):
            continue
        ids, par = t
        for node in range(len(ids)):
            kids = children(par, node)
            if not kids:
                continue
            rows.append(int(row0[b]) + node)
            seq.append(b)
            nt.append(len(kids))
            tg.append([int(ids[c - 1]) for c in kids] + [-1] * (NT - len(kids)))
            dst.append([nd + c - 1 for c in kids] + [-1] * (NT - len(kids)))
        nd += len(ids)
    return rows, seq, tg, nt, dst


# ---------------------------------------------------------------- exact laws
def first_law(p, tokens):
    """The law of the token emitted at one node whose children carry `tokens`
    (distinct, in child order) under p (dict id -> Fraction, summing to 1): a
    child's token where it is accepted, else the own draw from p without the
    rejected ones."""
    out = {}
    reach, rem, gone = Fraction(1), Fraction(1), set()
    for t in tokens:
        if reach == 0:
            break
        w = p.get(t, Fraction(0))
        a = w / rem  # rem > 0 while reach > 0
        out[t] = out.get(t, Fraction(0)) + reach * a
        reach *= 1 - a
        rem -= w
        gone.add(t)
    if reach > 0:
        for y, w in p.items():
            if y not in gone and w > 0:
                out[y] = out.get(y, Fraction(0)) + reach * w / rem
    return {k: v for k, v in out.items() if v > 0}


def plain_law(table, prefix, need):
    """token-by-token sampling: the law of the next `need` tokens after prefix"""
    if need == 0:
        return {(): Fraction(1)}
    out = {}
    for y, w in table(prefix).items():
        if w == 0:
            continue
        for tail, q in plain_law(table, prefix + (y,), need - 1).items():
            out[(y,) + tail] = out.get((y,) + tail, Fraction(0)) + w * q
    return out


def emitted_law(table, ids, parents, prefix, need, cur=0):
    """The joint law of the first `need` tokens a pass over the tree emits
    (accepted drafts, then the own token; what a pass does not reach comes
    from token-by-token sampling), coins integrated out."""
    if need == 0:
        return {(): Fraction(1)}
    p = table(prefix)
    out = {}

    def add(key, v):
        if v > 0:
            out[key] = out.get(key, Fraction(0)) + v

    reach, rem, gone = Fraction(1), Fraction(1), set()
    for c in children(parents, cur):
        if reach == 0:
            break
        t = ids[c - 1]
        w = p.get(t, Fraction(0))
        a = w / rem
        if a > 0:
            for tail, q in emitted_law(table, ids, parents, prefix + (t,), need - 1, c).items():
                add((t,) + tail, reach * a * q)
        reach *= 1 - a
        rem -= w
        gone.add(t)
    if reach > 0:
        for y, w in p.items():
            if y in gone or w == 0:
                continue
            for tail, q in plain_law(table, prefix + (y,), need - 1).items():
                add((y,) + tail, reach * w / rem * q)
    return out
