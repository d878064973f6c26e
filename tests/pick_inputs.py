"""Inputs and checkers for the greedy pick (the (max, argmax) row partials of
the LOGITS / SCORE epilogues and their reducers) in the two regimes the
uniform synthetic operands never reach.  Numpy only.

The contract (include/hip_paged_attn.h): a row's id is the lowest column of
the row's maximum, over the columns below N.

shifted(M, K, N, seed)
    today's operands with lb + 0.25 and W - 0.05: x stays zero-mean, the row
    sum of LN(x) is about 0.25 K, every logit moves by about -0.0125 K.  Every
    logit is negative, as with real GPT-2 weights, so a pad column of the last
    16-column tile (accumulator exactly 0.0: the packed weights' pad rows are
    zero) would win every row of a path that lost its `col < N` mask.
ties(M, K, N, E, O)
    exact, order-proof ties: row m of x is +1 at k = m % 2 and -1 at k = 2 +
    m % 2, zero elsewhere; lw = 1, lb = 0; W is zero but for columns k = 0, 1:
    W[n, 0] = -0.5 for n in E, W[n, 1] = -0.5 for n in O, -1 otherwise (a column
    in both sets is (-0.5, -0.5)).  Each row's sum is exactly 0, so its mean is
    0 in any arithmetic and LN(x) is +r at the +1, -r at the -1 (which meets
    W = 0) and exactly 0 elsewhere, r = 1/sqrt(2/K + 1e-5).  A logit is then
    ONE nonzero product, r W[n, m % 2], plus zeros: no rounding whatever the
    order of the sum, so even rows hold -r/2 on exactly the columns of E and
    -r elsewhere, odd rows the same on O, bit-equal in every kernel; the
    values are dyadic, so bf16 weights keep them.  (With a plain one-hot row
    LN(x) is nonzero at the other k too, and a column that is in E and in O
    would then differ from one that is in E alone by half of it: the sets
    below share columns.)  The pad columns' 0.0 lies above every live value.
    Expected pick: min(E) on even rows, min(O) on odd ones.
negative_logit_params(cfgd, seed, delta, beta)
    synth.params with wte[:, k] += delta u_k and lnfb[k] -= beta u_k, u = (+1,
    -1, +1, ...): sum u = 0, so no embedding row's mean moves, and every logit
    moves by about -delta beta C.

Checkers (AssertionError on a wrong answer; tests/test_pick_inputs.py feeds
each of them numpy-made wrong answers):
check_pick      0 <= id < N and id == the first argmax of the path's own logits
check_partials  every partial's column < N or the empty marker; its value the
                maximum of its live columns bit for bit, its column the lowest
                holding it; rows >= M hold no finite value
check_untouched rows with active <= 0 keep what they held
"""
import numpy as np

import synth
from gemm_bounds import bf16_operands, fp32_bound

EMPTY = 0x7FFFFFFF  # the column of a partial that saw no live column (hpa_logits.hip, hpa_fused.hip)


def ln64(x, w, b):
    """layernorm_forward in float64"""
    x = np.asarray(x, np.float64)
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + 1e-5) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def _product(x, W, lw, lb, w_bf16):
    a = ln64(x, lw, lb)
    if w_bf16:
        a, Wr, extra = bf16_operands(a, W)
        return a @ Wr.T, fp32_bound(a, Wr) + extra
    W64 = W.astype(np.float64)
    return a @ W64.T, fp32_bound(a, W64)


def shifted(M, K, N, seed, w_bf16=False):
    """dict(x, W, bias, lw, lb: fp32 operands; acc: the float64 product LN(x) W^T
    (of the bf16-rounded operands when w_bf16); bound: gemm_bounds.fp32_bound
    (plus bf16_operands' term))"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    lw = rng.uniform(0.8, 1.2, K).astype(np.float32)
    lb = (rng.uniform(-0.1, 0.1, K) + 0.25).astype(np.float32)
    W = (rng.uniform(-0.05, 0.05, (N, K)) - 0.05).astype(np.float32)
    acc, bound = _product(x, W, lw, lb, w_bf16)
    return dict(x=x, W=W, bias=np.zeros(N, np.float32), lw=lw, lb=lb, acc=acc, bound=bound, w_bf16=w_bf16)


def top2_margin(a):
    """per row: the maximum minus the second largest value"""
    p = np.partition(np.asarray(a), a.shape[-1] - 2, axis=-1)
    return p[..., -1] - p[..., -2]


def check_shifted_inputs(inp):
    """the condition on shifted()'s inputs, on the float64 product alone:
    every logit <= -1, at least M/2 distinct argmax ids, every row's top-2
    margin above twice the worst bound (the kernel's argmax is the float64
    one).  The margin is asked of fp32 weights only: with bf16 weights an A
    element near a rounding midpoint adds a bf16 ulp of it to its row's bound
    (gemm_bounds.bf16_operands), 20 times the fp32 bound, and nothing here
    compares a bf16 pick with the float64 argmax -- every pick is held to the
    path's own logits.  Returns (max, distinct ids, smallest margin, worst
    bound)."""
    acc, bound = inp["acc"], inp["bound"]
    M = acc.shape[0]
    ids = acc.argmax(-1)
    margin = top2_margin(acc)
    assert acc.max() <= -1.0, acc.max()
    assert len(set(ids.tolist())) >= M / 2, len(set(ids.tolist()))
    if not inp["w_bf16"]:
        assert np.all(margin > 2 * bound.max()), (float(margin.min()), float(bound.max()))
    return float(acc.max()), len(set(ids.tolist())), float(margin.min()), float(bound.max())


def tie_sets(N):
    """the column sets (E, O) for N = 1 (mod 16): (a) ties inside a tile,
    across adjacent tiles, across workgroups / rounds / super-tiles and in the
    lone live column of the last tile; (b) the last column alone against one
    far below it; (c) the two ends"""
    assert N % 16 == 1 and N > 64
    c = 4000 if N > 4002 else 16 * (N // 32)  # a tile's first two columns, far from both ends
    return dict(a=([7, 9, 16, c, c + 1, N - 2, N - 1], [9, 23, c + 1, N - 1]),
                b=([N - 1], [c + 1, N - 1]),
                c=([0], [N - 1]))


def ties(M, K, N, E, O):
    """dict(x, W, bias, lw, lb; acc: the float64 product; want: the expected id
    of every row; E, O sorted)"""
    E, O = sorted(E), sorted(O)
    x = np.zeros((M, K), np.float32)
    x[np.arange(M), np.arange(M) % 2] = 1.0
    x[np.arange(M), 2 + np.arange(M) % 2] = -1.0
    W = np.zeros((N, K), np.float32)
    W[:, :2] = -1.0
    W[E, 0] = -0.5
    W[O, 1] = -0.5
    lw, lb = np.ones(K, np.float32), np.zeros(K, np.float32)
    acc = ln64(x, lw, lb) @ W.astype(np.float64).T
    want = np.where(np.arange(M) % 2 == 0, E[0], O[0]).astype(np.int32)
    return dict(x=x, W=W, bias=np.zeros(N, np.float32), lw=lw, lb=lb, acc=acc, want=want, E=E, O=O)


def check_ties_inputs(inp):
    """the condition on ties()'s inputs (float64): even rows take their maximum
    on exactly E, odd rows on exactly O, at least 1 above every other column,
    and nothing is above -1"""
    acc = inp["acc"]
    N = acc.shape[1]
    for par, cols in ((0, inp["E"]), (1, inp["O"])):
        rows = acc[par::2]
        if not len(rows):
            continue
        other = np.ones(N, bool)
        other[cols] = False
        top = rows[:, cols]
        assert np.all(top == top[:, :1])  # the same single product
        assert np.all(top[:, :1] - rows[:, other] > 1.0)
    assert acc.max() <= -1.0


def check_tied_logits(own_logits, inp):
    """a path's stored logits on ties(): bit-equal on the expected columns of
    every row, strictly below there on every other column, all negative"""
    x = np.asarray(own_logits, np.float32)
    N = x.shape[1]
    assert np.all(x < 0)
    for par, cols in ((0, inp["E"]), (1, inp["O"])):
        rows = x[par::2]
        if not len(rows):
            continue
        other = np.ones(N, bool)
        other[cols] = False
        top = rows[:, cols]
        assert np.array_equal(top.view(np.uint32), np.broadcast_to(top[:, :1], top.shape).view(np.uint32))
        assert np.all(rows[:, other] < top[:, :1])


def check_pick(ids, own_logits, N):
    """ids (M,) against the path's own logits (M, N): 0 <= id < N, id == the
    lowest column of the row's maximum"""
    ids = np.asarray(ids).astype(np.int64)
    x = np.asarray(own_logits)
    assert x.shape == (len(ids), N), (x.shape, len(ids), N)
    assert np.all((ids >= 0) & (ids < N)), ids[(ids < 0) | (ids >= N)]
    want = x.argmax(-1)  # numpy returns the first
    bad = np.flatnonzero(ids != want)
    assert not len(bad), (bad[:8], ids[bad[:8]], want[bad[:8]])


def tile_owner_strided(ntiles, G):
    """tile t belongs to partial t % G (the 16-wave resident form)"""
    return np.arange(ntiles) % G


def tile_owner_runs(ntiles, G):
    """contiguous runs, the first ntiles % G one longer (the resident ring form)"""
    q, r = divmod(ntiles, G)
    return np.repeat(np.arange(G), q + (np.arange(G) < r))


def check_partials(part, own_logits, N, M, owner=None):
    """part (P, Mp, 2) float32: (value, the column's bits) per partial and row.
    own_logits (M, N): what the same launch stored.  owner: for every
    16-column tile the partial that covers it (None: partial t = tile t).
      * every column is < N, or EMPTY beside a value of -inf
      * rows < M: the value is the maximum of the partial's live columns, bit
        for bit, and the column the lowest one holding it; a partial with no
        live column is (-inf, EMPTY)
      * rows >= M hold no finite value"""
    part = np.ascontiguousarray(part, np.float32)
    P, Mp, two = part.shape
    assert two == 2 and Mp >= M
    val = part[..., 0]
    col = part[..., 1].copy().view(np.int32)
    ntiles = (N + 15) // 16
    assert np.all(((col >= 0) & (col < N)) | ((col == EMPTY) & (val == -np.inf))), \
        (np.argwhere(~(((col >= 0) & (col < N)) | (col == EMPTY)))[:4], N)
    assert not np.isfinite(val[:, M:]).any(), np.argwhere(np.isfinite(val[:, M:]))[:4]
    assert not np.isnan(val).any()
    x = np.full((M, ntiles * 16), -np.inf, np.float32)
    x[:, :N] = own_logits
    x = x.reshape(M, ntiles, 16)
    tmax = x.max(-1)                                       # (M, ntiles)
    tcol = x.argmax(-1) + 16 * np.arange(ntiles)[None, :]  # first within the tile
    if owner is None:
        assert P == ntiles, (P, ntiles)
        want_v, want_c = tmax.T, tcol.T
    else:
        owner = np.asarray(owner)
        assert owner.shape == (ntiles,) and owner.max() < P
        want_v = np.full((P, M), -np.inf, np.float32)
        want_c = np.full((P, M), EMPTY, np.int64)
        for p in range(P):
            t = np.flatnonzero(owner == p)  # ascending tiles: ascending columns
            if len(t):
                want_v[p] = tmax[:, t].max(-1)
                want_c[p] = tcol[np.arange(M), t[tmax[:, t].argmax(-1)]]
    got_v, got_c = val[:, :M], col[:, :M]
    bad = np.argwhere(got_v.view(np.uint32) != np.ascontiguousarray(want_v, np.float32).view(np.uint32))
    assert not len(bad), ("value", bad[:4], got_v[tuple(bad[0])], want_v[tuple(bad[0])])
    bad = np.argwhere(got_c != want_c)
    assert not len(bad), ("column", bad[:4], got_c[tuple(bad[0])], want_c[tuple(bad[0])])


def check_untouched(active, before, after):
    """rows b with active[b] <= 0 hold in `after` what they held in `before`
    (arrays with the row first); active None: every row is active"""
    if active is None:
        return
    off = np.asarray(active) <= 0
    b, a = np.asarray(before), np.asarray(after)
    assert b.shape == a.shape and len(b) == len(off)
    bad = np.flatnonzero([not np.array_equal(a[i], b[i]) for i in np.flatnonzero(off)])
    assert not len(bad), ("inactive rows written", np.flatnonzero(off)[bad][:8])


def negative_logit_params(cfgd, seed, delta, beta):
    """synth.params(cfgd, seed) with wte[:, k] += delta * u_k and lnfb[k] -=
    beta * u_k, u = (+1, -1, +1, ...).  sum(u) = 0 (C is even): no embedding
    row's mean moves; LNf(x) . wte[n] moves by about -beta * delta * C."""
    p = synth.params(cfgd, seed=seed).copy()
    V, C = cfgd["V"], cfgd["C"]
    assert C % 2 == 0
    u = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    off, sz = synth.offsets(cfgd), synth.sizes(cfgd)
    wte = p[off[0]:off[0] + sz[0]].reshape(V, C)
    wte += (delta * u).astype(np.float32)[None, :]
    p[off[15]:off[15] + sz[15]] -= (beta * u).astype(np.float32)
    return p


def check_negative_regime(logits, min_ids=8):
    """the condition on an engine case, on the oracle's logits (steps, B, V) of
    every row the test compares: every maximum <= -1 and at least min_ids
    distinct greedy ids over the run.  Returns (min, max, distinct ids)."""
    x = np.asarray(logits)
    x = x.reshape(-1, x.shape[-1])
    ids = set(x.argmax(-1).tolist())
    assert x.max() <= -1.0, x.max()
    assert len(ids) >= min_ids, len(ids)
    return float(x.min()), float(x.max()), len(ids)
