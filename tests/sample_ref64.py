"""float64 restatement of hpa_sample_filtered's rules (include/hip_paged_attn.h).

Per row x (fp32 logits) with temperature T, top-k k, top-p P and coin u:
  canonical order  tokens by (logit descending, index ascending)
  top-k            k = 0 or k >= V keeps everything, else the first k of the order
  probabilities    p_i = exp((x_i - max) / T) / sum over the top-k set
  top-p            the shortest canonical prefix inside the top-k set whose
                   mass is >= P; at least one token; P = 1 keeps the set
  n_kept, cut      the prefix length and the logit of its last token; kept =
                   every x > cut plus the lowest-indexed x == cut, n_kept in all
  draw             over the kept tokens in index order, renormalised: the first
                   kept index whose running cdf exceeds u; else the last kept
  T = 0            greedy: argmax, lowest index on ties; n_kept 1, cut = max
The coin is the reference's xorshift* generator in Python integers.

Everything here is computed in float64 from the fp32 logits; the checkers at
the bottom are shared by the raw-kernel and the engine tests.
"""
import numpy as np

_M64 = (1 << 64) - 1


def xorshift_u32(state):
    """(new state, 32 random bits): random_u32 of the reference"""
    s = int(state) & _M64
    s ^= s >> 12
    s ^= (s << 25) & _M64
    s ^= s >> 27
    return s, ((s * 0x2545F4914F6CDD1D) & _M64) >> 32


def coin(state):
    """(new state, u): random_f32, u = (r >> 8) / 2^24 in float32"""
    s, r = xorshift_u32(state)
    return s, np.float32(r >> 8) / np.float32(16777216.0)


def sanitise(T, k, P):
    """the device's reading of out-of-range settings"""
    T, P = np.float32(T), np.float32(P)
    if not (T >= 0) or np.isinf(T):
        T = np.float32(1)
    if k < 0:
        k = 0
    if not (P > 0 and P <= 1):
        P = np.float32(1)
    return T, int(k), P


class Row:
    """order: the canonical order; K: the top-k set's size (order[:K] is the
    exact set); M[i]: mass of order[:i + 1] within the top-k set (float64)"""

    def __init__(self, x, T, k):
        x = np.asarray(x, np.float32)
        V = x.size
        self.x, self.T = x, float(T)
        self.order = np.lexsort((np.arange(V), -x.astype(np.float64)))
        self.K = V if (k <= 0 or k >= V) else int(k)
        top = x[self.order[:self.K]].astype(np.float64)
        w = np.exp((top - float(x.max())) / self.T)
        self.M = np.cumsum(w) / w.sum()

    def n_kept(self, P):
        """the exact float64 prefix length"""
        if P >= 1:
            return self.K
        return min(self.K, int(np.searchsorted(self.M, float(P), side="left")) + 1)

    def admissible(self, P, tol):
        """every n with M[n-1] >= P - tol and (n == 1 or M[n-2] < P + tol)"""
        if P >= 1:
            return [self.K]
        P = float(P)
        lo = int(np.searchsorted(self.M, P - tol, side="left")) + 1  # smallest n with M[n-1] >= P - tol
        lo = min(lo, self.K)
        out = []
        n = lo
        while n <= self.K and (n == 1 or self.M[n - 2] < P + tol):
            if self.M[n - 1] >= P - tol:
                out.append(n)
            n += 1
        return out

    def cut(self, n):
        return self.x[self.order[n - 1]]


def kept_indices(x, n, cut):
    """the kept set (n, cut) defines, ascending: x > cut, then lowest-indexed x == cut"""
    x = np.asarray(x, np.float32)
    above = np.flatnonzero(x > cut)
    ties = np.flatnonzero(x == cut)[:max(0, n - above.size)]
    return np.sort(np.concatenate([above, ties]))


def index_cdf(x, kept, T):
    """float64 cdf over the kept tokens in index order, renormalised to their mass"""
    x = np.asarray(x, np.float32)
    w = np.exp((x[kept].astype(np.float64) - float(x.max())) / float(T))
    return np.cumsum(w) / w.sum()


def pick(x, T, k, P, u):
    """the exact float64 draw: (id, n_kept, cut)"""
    x = np.asarray(x, np.float32)
    T, k, P = sanitise(T, k, P)
    if T == 0:
        return int(np.argmax(x)), 1, x.max()
    row = Row(x, T, k)
    n = row.n_kept(P)
    cut = row.cut(n)
    kept = kept_indices(x, n, cut)
    c = index_cdf(x, kept, T)
    hit = np.flatnonzero(c > float(u))
    return int(kept[hit[0]] if hit.size else kept[-1]), n, cut


def tolerance(x, T):
    """max(4 e, 2^-20): e is the largest difference between the float64 cdf of
    the row and the one from its fp32 exp terms summed sequentially in fp32
    (the least accurate order a kernel would sensibly use); the factor 4
    covers expf and division differences"""
    x = np.asarray(x, np.float32)
    T = np.float32(T)
    w64 = np.exp((x.astype(np.float64) - float(x.max())) / float(T))
    c64 = np.cumsum(w64) / w64.sum()
    w32 = np.exp((x - x.max()) / T).astype(np.float32)
    c32 = np.cumsum(w32, dtype=np.float32)
    c32 = c32 / c32[-1]
    e = float(np.abs(c64 - c32.astype(np.float64)).max())
    return max(4 * e, 2.0 ** -20)


# ---------------------------------------------------------------- checkers
def check_cut(x, T, k, P, n, cut, tol, exact=False):
    """n_kept and cut of one sampled (T > 0) row, interval form.  exact: where
    no top-k cut is set the interval must admit one n only, the float64 one,
    and the device must report it"""
    T, k, P = sanitise(T, k, P)
    row = Row(x, T, k)
    assert 1 <= n <= row.K, (n, row.K)
    if P >= 1:
        assert n == row.K, (n, row.K)
    else:
        assert row.M[n - 1] >= float(P) - tol, (n, row.M[n - 1], P, tol)
        if n > 1:
            assert row.M[n - 2] < float(P) + tol, (n, row.M[n - 2], P, tol)
        if exact and row.K == row.x.size:  # (with a top-k cut P * K can sit on a boundary: equal, k = 50, P = 0.9)
            adm = row.admissible(P, tol)
            assert adm == [row.n_kept(P)], (adm, row.n_kept(P))
            assert n == adm[0], (n, adm)
    want = row.cut(n)
    assert np.float32(cut).tobytes() == np.float32(want).tobytes(), (cut, want)
    return row


def check_pick(x, T, n, cut, u, nxt, tol):
    """the id against the index-order cdf over the kept set (n, cut)"""
    kept = kept_indices(x, n, cut)
    assert kept.size == n, (kept.size, n)
    at = int(np.searchsorted(kept, nxt))
    assert at < kept.size and kept[at] == nxt, ("pick outside the kept set", nxt, n, cut)
    c = index_cdf(x, kept, T)
    lo = c[at - 1] if at > 0 else 0.0
    assert lo - tol <= float(u) < c[at] + tol, (nxt, lo, float(u), c[at], tol)


def check_pick_any(x, T, k, P, u, nxt, tol):
    """the id where the device's (n_kept, cut) are not visible (the engine):
    it must pass check_pick for an n the interval admits"""
    T, k, P = sanitise(T, k, P)
    if T == 0:
        assert nxt == int(np.argmax(x)), (nxt, int(np.argmax(x)))
        return
    row = Row(x, T, k)
    errs = []
    for n in row.admissible(P, tol):
        try:
            check_pick(x, T, n, row.cut(n), u, nxt, tol)
            return
        except AssertionError as e:  # try the next admissible n
            errs.append(e)
    raise AssertionError(("no admissible n explains the pick", nxt, errs))
