"""Speculative sampling with point-mass drafts, restated on sample_ref64
(the rule of gpt2_decode_verify_sampled, include/paged_infer.h).

p = the distribution mode 2 draws from at a row: temperature, top-k and top-p
applied as hpa_sample_filtered defines the kept set and the masses.  A draft d
after that row is accepted with probability p(d); at a rejection the model's own
token comes from the residual: p with d removed and the rest renormalised,
walked in index order like every draw.

  [y = d] p(d) + (1 - p(d)) residual_d(y) = p(y)      for every y and every d

so the emitted token is distributed as a plain draw from p.

The walk itself runs on the device in integers: the coin is j = u32 >> 8
(u = j / 2^24) and a draft with fixed-point masses (w_target, w_total) is
accepted iff w_target * 2^24 > w_total * j.  accept_walk restates it in Python
integers, one xorshift state per sequence.
"""
import numpy as np

import sample_ref64 as sr


def kept_set(x, T, k, P):
    """(kept indices ascending, n_kept, cut) in float64; T = 0: the argmax alone"""
    x = np.asarray(x, np.float32)
    T, k, P = sr.sanitise(T, k, P)
    if T == 0:
        return np.array([int(np.argmax(x))]), 1, x.max()
    row = sr.Row(x, T, k)
    n = row.n_kept(P)
    cut = row.cut(n)
    return sr.kept_indices(x, n, cut), n, cut


def masses(x, kept, T):
    """float64 probabilities of the kept tokens (ascending index), summing to 1"""
    x = np.asarray(x, np.float32)
    if float(T) == 0:
        return np.ones(len(kept)) / len(kept)
    w = np.exp((x[kept].astype(np.float64) - float(x.max())) / float(T))
    return w / w.sum()


def accept_prob(x, T, k, P, d):
    """p(d): the mass mode 2 gives id d at this row; 0 outside the kept set"""
    kept, _, _ = kept_set(x, T, k, P)
    at = np.flatnonzero(kept == int(d))
    if at.size == 0:
        return 0.0
    return float(masses(x, kept, sr.sanitise(T, k, P)[0])[at[0]])


def accept_prob_kept(x, T, kept, d):
    """p(d) over a given kept set (the device's own (n_kept, cut))"""
    at = np.flatnonzero(np.asarray(kept) == int(d))
    if at.size == 0:
        return 0.0
    return float(masses(x, kept, T)[at[0]])


def residual(x, T, kept, d):
    """(ids, cdf): the kept set without d, ascending, and the float64 cdf of its
    renormalised masses.  d outside the kept set removes nothing; removing the
    only kept id is dropped (the id stays)."""
    kept = np.asarray(kept)
    rest = kept[kept != int(d)]
    if rest.size == 0:
        rest = kept
    m = masses(x, kept, T)[np.isin(kept, rest)]
    return rest, np.cumsum(m) / m.sum()


def check_pick_residual(x, T, n, cut, d, u, nxt, tol):
    """sample_ref64.check_pick on the residual cdf: nxt is kept, is not d, and
    its cdf interval holds u"""
    kept = sr.kept_indices(x, n, cut)
    assert kept.size == n, (kept.size, n)
    rest, c = residual(x, T, kept, d)
    at = int(np.searchsorted(rest, nxt))
    assert at < rest.size and rest[at] == nxt, ("pick outside the residual set", nxt, d, n, cut)
    lo = c[at - 1] if at > 0 else 0.0
    assert lo - tol <= float(u) < c[at] + tol, (nxt, d, lo, float(u), c[at], tol)


def accepts(w_target, w_total, j):
    """the integer test: u = j / 2^24 < w_target / w_total"""
    return int(w_target) * (1 << 24) > int(w_total) * int(j)


def accept_walk(state, w_target, w_total, drafts):
    """One sequence's walk.  w_target / w_total / drafts: per drafted row.
    Returns (new state, n_accepted, rejected draft or -1, the coins j drawn)."""
    coins = []
    a, rejected = 0, -1
    for wt, ws, d in zip(w_target, w_total, drafts):
        state, r = sr.xorshift_u32(state)
        j = r >> 8
        coins.append(j)
        if not accepts(wt, ws, j):
            rejected = int(d)
            break
        a += 1
    return state, a, rejected, coins
