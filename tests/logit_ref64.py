"""float64 restatement of the logit processors (include/paged_infer.h,
hpa_logits_process in include/hip_paged_attn.h) and its tolerance.

For a row b and column t, x = the raw fp32 logit, c = count[b][t], the
processed logit is, in this order,

    if c > 0:  x = x / r if x > 0 else x * r          repetition (r > 0, 1 = off)
    x = x - f * c - (p if c > 0 else 0)               frequency, presence (0 = off)
    if t is in the bias list:  x = x + bias           finite, or -inf = a ban

count[b][t] = the positions p in [from_pos, pos) with history[p] == t.

Tolerance.  The device computes the same steps in fp32.  Each of its at most
four roundings (the divide or multiply, f * c, the two subtractions / the add)
is within 2^-24 of a partial result that S = |x'| + |f c| + |p| + |bias| bounds
(x' the value after the repetition step), so the fp32 result lies within
2^-22 S of the float64 one; the bar is twice that, tol = 2^-21 S, per element.
A reference value of -inf (a ban, or a raw -inf) must be -inf on the device.
"""
import numpy as np

BIAS_MAX = 300


def counts_from(history, from_pos, pos, V):
    """count[t] over the window [from_pos, pos) of one sequence's fed tokens"""
    h = np.asarray(history, np.int64)[max(0, int(from_pos)):max(0, int(pos))]
    return np.bincount(h, minlength=V).astype(np.int64)


def process(x, counts, r=1.0, p=0.0, f=0.0, bias_ids=(), bias_vals=()):
    """one row: (processed float64 [V], tol float64 [V])"""
    x32 = np.asarray(x, np.float32)
    x = x32.astype(np.float64)
    c = np.asarray(counts).astype(np.float64)
    r, p, f = float(np.float32(r)), float(np.float32(p)), float(np.float32(f))
    seen = c > 0
    with np.errstate(invalid="ignore"):
        xr = np.where(seen, np.where(x > 0, x / r, x * r), x)
        fc = f * c
        pp = np.where(seen, p, 0.0)
        y = xr - fc - pp
        bias = np.zeros_like(x)
        ids = np.asarray(bias_ids, np.int64).reshape(-1)
        bias[ids] = np.asarray(bias_vals, np.float32).astype(np.float64).reshape(-1)
        y[ids] = y[ids] + bias[ids]  # the listed columns only: an unlisted -0 keeps its sign
        S = np.abs(xr) + np.abs(fc) + np.abs(pp) + np.where(np.isfinite(bias), np.abs(bias), 0.0)
    return y, 2.0 ** -21 * S


def winner(y):
    """the argmax, lowest index on ties; 0 for a row with nothing above -inf"""
    y = np.asarray(y, np.float64)
    if not np.any(y > -np.inf):
        return 0
    return int(np.argmax(y))


def lead(y, tol):
    """(winner, lead over the best other column, 2 * the larger tol of the two);
    the lead is inf where there is no other finite column"""
    y = np.asarray(y, np.float64)
    w = winner(y)
    rest = y.copy()
    rest[w] = -np.inf
    if not np.any(rest > -np.inf):
        return w, np.inf, 0.0
    ru = int(np.argmax(rest))
    return w, float(y[w] - y[ru]), 2.0 * float(max(tol[w], tol[ru]))


def assert_close(dev, y, tol, what=""):
    """every device element within tol of the reference; -inf where it is -inf"""
    dev = np.asarray(dev, np.float32).astype(np.float64)
    ninf = np.isneginf(y)
    assert np.array_equal(np.isneginf(dev), ninf), (what, "the -inf columns differ")
    assert not np.isnan(dev).any(), (what, "NaN")
    fin = ~ninf
    err = np.abs(dev[fin] - y[fin])
    bad = err > tol[fin]
    assert not bad.any(), (what, float(err.max()), np.flatnonzero(fin)[np.flatnonzero(bad)[:4]])
    return float((err / np.maximum(tol[fin], 1e-300)).max()) if err.size else 0.0


# ---------------------------------------------------------------- the kernel test's fixed inputs
# row kinds of tests/test_gpu_logit_process.py
NEUTRAL, REPETITION, PRES_FREQ, BIAS_LAST, BIAS_FIRST, ALL_BUT_ONE, ALL_BANNED, INACTIVE = range(8)

# (V, row kinds) of every launch: V = 1000 (aligned rows) and 1003 (odd stride:
# the head / tail differ per row) at 5 rows, V = 50257 at 3 rows
KERNEL_CASES = [
    (1000, (NEUTRAL, REPETITION, PRES_FREQ, BIAS_LAST, INACTIVE)),
    (1000, (BIAS_FIRST, ALL_BUT_ONE, INACTIVE, ALL_BANNED, NEUTRAL)),
    (1003, (NEUTRAL, REPETITION, PRES_FREQ, BIAS_LAST, INACTIVE)),
    (1003, (ALL_BANNED, BIAS_FIRST, ALL_BUT_ONE, INACTIVE, PRES_FREQ)),
    (50257, (NEUTRAL, BIAS_LAST, INACTIVE)),
    (50257, (REPETITION, ALL_BUT_ONE, PRES_FREQ)),
    (50257, (BIAS_FIRST, ALL_BANNED, REPETITION)),
]


def kernel_case(V, kinds, seed=0):
    """the inputs of one launch: dict of x [n][V] fp32, counts [n][V] uint16,
    r, p, f [n] fp32, bias_ids [n][300] int32, bias_vals [n][300] fp32, bias_n
    [n] int32, active [n] int32"""
    n = len(kinds)
    rng = np.random.default_rng(1000 * V + 17 * seed + sum((i + 1) * k for i, k in enumerate(kinds)))
    x = (rng.standard_normal((n, V)) * 3).astype(np.float32)
    counts = np.zeros((n, V), np.uint16)
    r, p, f = np.ones(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    ids = np.zeros((n, BIAS_MAX), np.int32)
    vals = np.zeros((n, BIAS_MAX), np.float32)
    nb = np.zeros(n, np.int32)
    active = np.ones(n, np.int32)
    for b, kind in enumerate(kinds):
        cols = rng.permutation(V)
        if kind == NEUTRAL:  # counts present, the maximum planted at two columns: the lower one wins
            counts[b, cols[:200]] = rng.integers(1, 50, 200)
            lo, hi = sorted(int(c) for c in cols[200:202])
            x[b, lo] = x[b, hi] = np.float32(x[b].max() + 1.0)
            counts[b, hi] = 3
        elif kind == REPETITION:  # 1.3 alone; the counted tokens include the raw maximum
            r[b] = 1.3
            counts[b, cols[:300]] = rng.integers(1, 9, 300)
            counts[b, int(np.argmax(x[b]))] = 2
            counts[b, int(np.argmin(x[b]))] = 1
        elif kind == PRES_FREQ:  # counts from 1 to 1000
            p[b], f[b] = 0.6, 0.02
            k = min(V // 2, 1000)
            counts[b, cols[:k]] = rng.integers(1, 1001, k)
            counts[b, cols[0]], counts[b, cols[1]] = 1, 1000
        elif kind in (BIAS_LAST, BIAS_FIRST):  # 300 entries: the raw argmax banned, one column lifted to the top
            lift = V - 1 if kind == BIAS_LAST else 0
            top = int(np.argmax(x[b]))
            if top == lift:
                x[b, lift] -= 1.0
                top = int(np.argmax(x[b]))
            r[b], p[b], f[b] = 1.1, 0.25, 0.01
            counts[b, cols[:100]] = rng.integers(1, 20, 100)
            others = [int(c) for c in cols if c not in (top, lift)][:BIAS_MAX - 2]
            ids[b] = np.array([top, lift] + others, np.int32)
            vals[b] = rng.uniform(-4, 4, BIAS_MAX).astype(np.float32)
            vals[b, 0], vals[b, 1] = -np.inf, 50.0
            vals[b, 2:40] = -np.inf
            nb[b] = BIAS_MAX
        elif kind in (ALL_BUT_ONE, ALL_BANNED):  # beyond 300 + 1 columns the raw row is -inf already
            live = np.sort(cols[:BIAS_MAX + 1])
            row = np.full(V, -np.inf, np.float32)
            row[live] = x[b, live]
            x[b] = row
            keep = int(live[BIAS_MAX // 2])
            banned = [int(c) for c in live if c != keep]
            ids[b] = np.array(banned, np.int32)
            vals[b] = -np.inf
            nb[b] = BIAS_MAX
            counts[b, live[:50]] = rng.integers(1, 5, 50)
            p[b], f[b] = 0.5, 0.1
            if kind == ALL_BANNED:
                x[b, keep] = -np.inf
        elif kind == INACTIVE:
            active[b] = 0
            r[b], p[b], f[b] = 1.5, 1.0, 1.0
            counts[b, cols[:100]] = 7
            ids[b, :3], vals[b, :3], nb[b] = (1, 2, 3), (5.0, -np.inf, 1.0), 3
    return dict(x=x, counts=counts, r=r, p=p, f=f, bias_ids=ids, bias_vals=vals, bias_n=nb, active=active)


def kernel_reference(case):
    """per row: (processed float64, tol) of kernel_case's inputs"""
    out = []
    for b in range(case["x"].shape[0]):
        n = int(case["bias_n"][b])
        out.append(process(case["x"][b], case["counts"][b], case["r"][b], case["p"][b], case["f"][b],
                           case["bias_ids"][b, :n], case["bias_vals"][b, :n]))
    return out
