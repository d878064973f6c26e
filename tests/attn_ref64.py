"""Float64 reference of the paged attention, its error unit, and the case
sets that aim a peaked softmax at the kernels' edges.  Numpy only.

Reference (one query of one head; q fp32, K and V the values the pool holds:
round_pool of what was drawn), all in float64:

    s_j = q.k_j / 8                  a_j = sum_i |q_i k_ji| / 8
    M   = max(-10000, max_j s_j)     p_j = exp(s_j - M)      Z = sum_j p_j
    out = sum_j p_j v_j / Z          (0 where Z == 0)
    W_d = sum_j p_j |v_jd| / Z
    E   = max a_j over the keys with p_j / Z >= 2^-24
    unit_d = 2^-24 (1 + E) W_d  +  ctx 2^-126 max|V|
    ratio  = max_d |got_d - out_d| / unit_d

E carries the rounding of an fp32 score (the folded log2(e)/8 factor and the
floor -10000 log2(e) included); the last term of unit_d covers weights that
are flushed denormals.  The floor is the fp32 rule of the code this project
restates (maxval = -10000, expf underflows, expsum == 0 gives a zero output),
so p_j is exactly 0 for s_j - M <= -120, and `attend` asserts that no s_j - M
lies in (-120, -80): there a float64 p and an fp32 p could disagree about
being zero.  A prefill query row t of sequence b is the same function with
ctx = start[b] + t + 1.

Cases (K, V ~ U(-1, 1) rounded to the pool's dtype unless said otherwise):

    hot(j)           q = 15 K[j]: key j wins by tens of nats, out ~ V[j]
    pair(j, j+1)     q = 15 (K[j] + K[j+1]): two comparable weights
                     (15, or the next of 13, 11, 9 that keeps every score out
                     of the band above: _aimed)
    ramp_up / _down  K = 0.2 noise + t_j u (noise orthogonal to the unit
                     vector u), q = 600 u: scores 75 t_j, linear in j over
                     300 nats, except that depths in (60, 140) nats below the
                     top are moved 90 nats further down (the band above).  In
                     ramp_up every tile raises the running max; in ramp_down
                     the max is in the first tile and later tiles, waves and
                     split ranges bring partials that underflow to 0.
    below_floor_one  q = -20100 u; one key 4 u (score -10050, exact in every
                     pool dtype), the rest (5 + U(0, .5)) u + 0.2 noise
                     (scores <= -12000): that key's V through a tiny normal l
    below_floor_all  the same without the one key: output exactly 0
    uniform          q ~ U(-2, 2): the regime of the older tests, a control

`positions(ctx, P, NW, S)` is where hot and pair cases put their keys for a
launch of NW waves and S context ranges: 0, 1, P-1, P, 62..65, ctx-2, ctx-1,
the first and last token of each wave's last tile (per range), and
64 it0 - 1, 64 it0 of every range (it0 = sr n_tiles / S as the kernel cuts).
"""
import numpy as np

import synth
from pagedattn import HPA_BF16, HPA_F32, HPA_FP8, round_bf16, round_fp8

HS = 64
NH = 2
C = NH * HS
FLOOR = -10000.0
EPS = 2.0 ** -24
TINY = 2.0 ** -126
CONTEXTS = (1, 2, 63, 64, 65, 128, 129, 257, 513, 1000, 1024)  # 64 NW + 1 for NW = 1, 2, 4, 8 included
LAUNCHES = ((1, 1), (4, 1), (8, 1), (4, 2), (8, 3), (2, 16))   # (waves, splits)
K_SCALE = np.array([0.5, 2.0], np.float32)  # fp8 pools: per-head scales, none of them 1
V_SCALE = np.array([2.0, 0.5], np.float32)
KINDS = ("uniform", "hot", "pair", "ramp_up", "ramp_down", "below_floor_one", "below_floor_all")


class BandError(AssertionError):
    """an input whose s_j - M lies where float64 and fp32 may disagree about p_j == 0"""


# ---------------------------------------------------------------- the reference
class Ref:
    """out, unit (n, 64); E, wmax (largest softmax weight) (n,)"""

    def __init__(self, out, unit, E, wmax):
        self.out, self.unit, self.E, self.wmax = out, unit, E, wmax


def attend(Q, K, V, ctx=None):
    """Q (n, 64) fp32 queries of one head over one sequence's K, V (m, 64);
    ctx (n,) keys each query sees (default: all m)."""
    Q = np.asarray(Q, np.float64).reshape(-1, HS)
    K = np.asarray(K, np.float64)
    V = np.asarray(V, np.float64)
    n, m = Q.shape[0], K.shape[0]
    ctx = np.full(n, m) if ctx is None else np.asarray(ctx).reshape(n)
    assert ctx.min() >= 1 and ctx.max() <= m
    seen = np.arange(m)[None, :] < ctx[:, None]
    assert np.isfinite(K).all() and np.isfinite(V).all() and np.isfinite(Q).all()
    s = Q @ K.T / 8.0
    a = np.abs(Q) @ np.abs(K).T / 8.0
    M = np.maximum(FLOOR, np.where(seen, s, -np.inf).max(1))
    d = s - M[:, None]
    band = seen & (d > -120.0) & (d < -80.0)
    if band.any():
        i, j = np.argwhere(band)[0]
        raise BandError(f"query {i} key {j}: s - M = {d[i, j]:.2f} inside (-120, -80)")
    p = np.where(seen & (d >= -80.0), np.exp(np.minimum(d, 0.0)), 0.0)
    Z = p.sum(1)
    inv = np.where(Z > 0, 1.0 / np.where(Z > 0, Z, 1.0), 0.0)
    w = p * inv[:, None]
    out = w @ V
    W = w @ np.abs(V)
    E = np.where(w >= EPS, a, 0.0).max(1)
    vmax = np.where(seen, np.abs(V).max(1)[None, :], 0.0).max(1)
    unit = EPS * (1.0 + E)[:, None] * W + (ctx * TINY * vmax)[:, None]
    return Ref(out, unit, E, w.max(1))


def ratio(got, ref):
    """max_d |got - out| / unit per query; inf where got is not finite"""
    got = np.asarray(got, np.float64).reshape(ref.out.shape)
    r = (np.abs(got - ref.out) / ref.unit).max(1)
    return np.where(np.isfinite(got).all(1), r, np.inf)


# ---------------------------------------------------------------- fp32 restatement of the reference code
def attend_f32(Q, K, V, ctx=None):
    """the arithmetic the project restates, in numpy fp32: sequential dot over
    the 64 dims, maxval from -10000, expf, sequential expsum, weights times
    1 / expsum (0 where expsum == 0), sequential weighted sum of V"""
    Q = np.asarray(Q, np.float32).reshape(-1, HS)
    K = np.asarray(K, np.float32)
    V = np.asarray(V, np.float32)
    n, m = Q.shape[0], K.shape[0]
    ctx = np.full(n, m) if ctx is None else np.asarray(ctx).reshape(n)
    seen = np.arange(m)[None, :] < ctx[:, None]
    val = np.zeros((n, m), np.float32)
    for i in range(HS):
        val += Q[:, i, None] * K[None, :, i]
    val *= np.float32(1.0) / np.sqrt(np.float32(HS))
    maxval = np.maximum(np.float32(FLOOR), np.where(seen, val, -np.inf).max(1)).astype(np.float32)
    with np.errstate(under="ignore"):
        e = np.where(seen, np.exp(np.where(seen, val - maxval[:, None], 0).astype(np.float32)), 0).astype(np.float32)
        expsum = np.cumsum(e, 1, dtype=np.float32)[np.arange(n), ctx - 1]
        inv = np.where(expsum == 0, 0, np.float32(1.0) / np.where(expsum == 0, 1, expsum)).astype(np.float32)
        att = e * inv[:, None]
        out = np.zeros((n, HS), np.float32)
        for i0 in range(0, n, 16):  # (16, m, 64) at a time
            out[i0:i0 + 16] = np.cumsum(att[i0:i0 + 16, :, None] * V[None], 1, dtype=np.float32)[:, -1]
    return out


# ---------------------------------------------------------------- online-softmax restatement and its mutations
MUTATIONS = ("drop_last", "drop_first", "next_at_tile_edge", "max_from_minus_inf", "no_alpha", "stale_times_zero")


def attend_online(q, K, V, ctx, mutate=None, tile=64):
    """one query, float64, in the kernels' form: 64-key tiles folded into a
    running (m, l, acc) from m = -10000.  K, V may have more than ctx rows
    (stale slots; NaN in the poisoned pools).  mutate: one of MUTATIONS, each
    a way a kernel could be subtly wrong."""
    q = np.asarray(q, np.float64)
    K = np.asarray(K, np.float64)
    V = np.asarray(V, np.float64)
    m_run = -np.inf if mutate == "max_from_minus_inf" else FLOOR
    l = 0.0
    acc = np.zeros(HS)
    lo = 1 if mutate == "drop_first" else 0
    hi = ctx - 1 if mutate == "drop_last" else ctx
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, ctx, tile):
            idx = np.arange(t0, min(t0 + tile, K.shape[0]))
            src = idx.copy()
            if mutate == "next_at_tile_edge":
                edge = (idx % tile == tile - 1) & (idx + 1 < ctx)
                src[edge] += 1
            valid = (idx >= lo) & (idx < hi)
            if mutate == "stale_times_zero":  # the slot's score masked, its V row still multiplied
                s = np.where(valid, K[src] @ q / 8.0, -np.inf)
                v = V[src]
            else:
                s = np.where(valid, np.where(valid[:, None], K[src], 0.0) @ q / 8.0, -np.inf)
                v = np.where(valid[:, None], V[src], 0.0)
            mn = max(m_run, s.max()) if s.size else m_run
            if mn == -np.inf:
                continue
            alpha = 1.0 if mutate == "no_alpha" else np.exp(m_run - mn)
            d = s - mn
            p = np.where(d >= -100.0, np.exp(np.maximum(d, -100.0)), 0.0)
            l = l * alpha + p.sum()
            acc = acc * alpha + p @ v
            m_run = mn
    return acc / l if l != 0.0 else np.zeros(HS)


# ---------------------------------------------------------------- positions
def tile_ranges(ctx, S):
    """[it0, it1) of every context range, as paged_attn_decode_f32 cuts them"""
    n = (ctx + 63) >> 6
    return [(0, n)] if S == 1 else [(sr * n // S, (sr + 1) * n // S) for sr in range(S)]


def positions(ctx, P, NW, S):
    """sorted key positions in [0, ctx) at the edges of a launch of NW waves and S ranges"""
    pos = [0, 1, P - 1, P, 62, 63, 64, 65, ctx - 2, ctx - 1]
    for it0, it1 in tile_ranges(ctx, S):
        pos += [64 * it0 - 1, 64 * it0]
        for w in range(NW):  # wave w: tiles it0 + w, it0 + w + NW, ... < it1
            if it0 + w < it1:
                last = it0 + w + (it1 - 1 - it0 - w) // NW * NW
                pos += [64 * last, 64 * last + 63]
    return sorted({min(max(int(p), 0), ctx - 1) for p in pos})


def launch_positions(ctx, P, launches=LAUNCHES):
    """the union over the launches a case set serves"""
    return sorted({p for NW, S in launches for p in positions(ctx, P, NW, S)})


# ---------------------------------------------------------------- case sets
def round_pool(a, dtype, scale=None):
    """the values a pool of `dtype` holds for a (rows, NH * 64); scale (NH,): an fp8 pool's per-head scales"""
    a = np.asarray(a, np.float32)
    if dtype == HPA_BF16:
        return round_bf16(a)
    if dtype == HPA_FP8:
        return round_fp8(a.reshape(-1, NH, HS), np.asarray(scale, np.float32)[None, :, None]).reshape(a.shape)
    assert dtype == HPA_F32
    return a


def _unit_vector(rng):
    return (rng.integers(0, 2, HS) * 2 - 1) / 8.0  # |u| = 1, every component +-1/8


def _perp_noise(rng, n, u):
    z = rng.uniform(-1, 1, (n, HS))
    return z - (z @ u)[:, None] * u[None, :]


def _ramp_keys(rng, ctx, up):
    u = _unit_vector(rng)
    depth = np.linspace(0.0, 300.0, ctx) if ctx > 1 else np.zeros(1)
    depth = np.where((depth > 60.0) & (depth < 140.0), depth + 90.0, depth)
    if up:
        depth = depth[::-1]
    t = 4.0 - depth / 75.0
    return 0.2 * _perp_noise(rng, ctx, u) + t[:, None] * u[None, :], (600.0 * u).astype(np.float32)


def _floor_keys(rng, ctx, one):
    """one: position of the key at -10050, or None (every key <= -12000)"""
    u = _unit_vector(rng)
    t = 5.0 + rng.uniform(0, 0.5, ctx)
    k = 0.2 * _perp_noise(rng, ctx, u) + t[:, None] * u[None, :]
    if one is not None:
        k[one] = 4.0 * u
    return k, (-20100.0 * u).astype(np.float32)


def _aimed(Kh, vec):
    """q = f vec, f = 15 -- or the next of 13, 11, 9 at which no key's score
    lies in the band (-120, -80) below the top (a few pair queries at long
    contexts need it)"""
    s = np.asarray(Kh, np.float64) @ np.asarray(vec, np.float64) / 8.0
    d = s - s.max()
    for f in (15.0, 13.0, 11.0, 9.0):
        if not ((f * d > -121.0) & (f * d < -79.0)).any():
            return (f * np.asarray(vec, np.float64)).astype(np.float32)
    raise BandError("no factor keeps the scores out of the band")


class Cases:
    """seqs: [(K, V)] (ctx, C) fp32, the pool's values; rows: per query row
    its sequence, ctx, q (C,) and per-head kind labels"""

    def __init__(self):
        self.seqs, self.seq, self.ctx, self.q, self.kind = [], [], [], [], []

    def add_row(self, seq, ctx, q, kinds):
        self.seq.append(seq)
        self.ctx.append(ctx)
        self.q.append(np.asarray(q, np.float32).reshape(C))
        self.kind.append(tuple(kinds))

    def finish(self):
        self.seq = np.array(self.seq, np.int32)
        self.ctx = np.array(self.ctx, np.int32)
        self.q = np.stack(self.q).astype(np.float32)
        self._ref = None
        return self

    def reference(self):
        """(out, unit) (rows, C), E and wmax (rows, NH); computed once"""
        if self._ref is None:
            B = len(self.seq)
            out, unit = np.zeros((B, C)), np.zeros((B, C))
            E, wmax = np.zeros((B, NH)), np.zeros((B, NH))
            for si, (K, V) in enumerate(self.seqs):
                rows = np.nonzero(self.seq == si)[0]
                if not rows.size:
                    continue
                for h in range(NH):
                    c = slice(h * HS, (h + 1) * HS)
                    r = attend(self.q[rows, c], K[:, c], V[:, c], self.ctx[rows])
                    out[rows, c], unit[rows, c], E[rows, h], wmax[rows, h] = r.out, r.unit, r.E, r.wmax
            self._ref = (out, unit, E, wmax)
        return self._ref

    def ratios(self, got):
        """(rows, NH): the worst ratio of every (row, head); inf where got is not finite"""
        out, unit = self.reference()[:2]
        got = np.asarray(got, np.float64).reshape(out.shape)
        with np.errstate(invalid="ignore"):
            r = (np.abs(got - out) / unit).reshape(-1, NH, HS).max(2)
        return np.where(np.isfinite(got).reshape(-1, NH, HS).all(2), r, np.inf)

    def worst_by_kind(self, ratios):
        kinds = np.array(self.kind)
        return {k: float(ratios[kinds == k].max()) for k in KINDS if (kinds == k).any()}


def _scales(dtype):
    return (K_SCALE, V_SCALE) if dtype == HPA_FP8 else (None, None)


def decode_cases(P, dtype, launches=LAUNCHES, contexts=CONTEXTS, seed=0):
    """one batch of decode rows for a pool of page size P and `dtype`, serving every launch of `launches`"""
    ks, vs = _scales(dtype)
    cs = Cases()

    def add_seq(k, v):
        cs.seqs.append((round_pool(k, dtype, ks), round_pool(v, dtype, vs)))
        return len(cs.seqs) - 1

    for ctx in contexts:
        rng = np.random.default_rng([seed, ctx, P])
        # uniform K, V: hot, pair and uniform rows
        su = add_seq(rng.uniform(-1, 1, (ctx, C)), rng.uniform(-1, 1, (ctx, C)))
        K = cs.seqs[su][0]
        pos = launch_positions(ctx, P, launches)
        for r in range((len(pos) + NH - 1) // NH):  # a different j for each head of a row
            js = [pos[(NH * r + h) % len(pos)] for h in range(NH)]
            cs.add_row(su, ctx, np.concatenate([_aimed(K[:, h * HS:(h + 1) * HS], K[j, h * HS:(h + 1) * HS])
                                                for h, j in enumerate(js)]),
                       ["hot"] * NH)
        pp = [j for j in pos if j + 1 < ctx]
        for r in range((len(pp) + NH - 1) // NH):
            js = [pp[(NH * r + h + 1) % len(pp)] for h in range(NH)]
            cs.add_row(su, ctx, np.concatenate([_aimed(K[:, h * HS:(h + 1) * HS],
                                                       K[j, h * HS:(h + 1) * HS] + K[j + 1, h * HS:(h + 1) * HS])
                                                for h, j in enumerate(js)]), ["pair"] * NH)
        cs.add_row(su, ctx, rng.uniform(-2, 2, C), ["uniform"] * NH)
        # ramps: both orders of (up, down) over the two heads
        for ups in ((True, False), (False, True)):
            kq = [_ramp_keys(rng, ctx, up) for up in ups]
            s = add_seq(np.concatenate([k for k, _ in kq], 1), rng.uniform(-1, 1, (ctx, C)))
            cs.add_row(s, ctx, np.concatenate([q for _, q in kq]), ["ramp_up" if up else "ramp_down" for up in ups])
        # below the floor: the one key at ctx - 1 / at the first token of the last tile
        for ones in ((ctx - 1, None), (None, (ctx - 1) // 64 * 64)):
            kq = [_floor_keys(rng, ctx, one) for one in ones]
            s = add_seq(np.concatenate([k for k, _ in kq], 1), rng.uniform(-1, 1, (ctx, C)))
            cs.add_row(s, ctx, np.concatenate([q for _, q in kq]),
                       ["below_floor_all" if one is None else "below_floor_one" for one in ones])
    return cs.finish()


PREFILL_STARTS = (0, 5, 70, 250)


def prefill_hot_choices(start, t):
    """keys a hot query row t may aim at: 0, start - 1, start, its own key
    start + t (the last it sees), start + t - 1, and the 16-key tile edges
    below start + t"""
    qpos = start + t
    e = qpos // 16 * 16
    c = [0, start - 1, start, qpos, qpos - 1, e - 1, e, e - 16, e - 17]
    return sorted({j for j in c if 0 <= j <= qpos})


def prefill_cases(dtype, starts=PREFILL_STARTS, lens=(130, 130, 130, 130), seed=1):
    """query rows t = 0..lens[b]-1 of sequence b at positions starts[b] + t,
    packed in sequence order; row kinds cycle hot (6 of 8), pair, uniform"""
    ks, vs = _scales(dtype)
    cs = Cases()
    for b, (start, n) in enumerate(zip(starts, lens)):
        rng = np.random.default_rng([seed, b, start, n])
        m = start + n
        K = round_pool(rng.uniform(-1, 1, (m, C)), dtype, ks)
        V = round_pool(rng.uniform(-1, 1, (m, C)), dtype, vs)
        cs.seqs.append((K, V))
        for t in range(n):
            qpos = start + t
            kind = ("hot", "hot", "pair", "hot", "hot", "uniform", "hot", "hot")[(t + 3 * b) % 8]
            if kind == "pair" and qpos == 0:
                kind = "hot"
            if kind == "uniform":
                q = rng.uniform(-2, 2, C)
            else:
                q = np.zeros(C, np.float32)
                for h in range(NH):
                    c = slice(h * HS, (h + 1) * HS)
                    ch = prefill_hot_choices(start, t)
                    if kind == "pair":
                        ch = [j for j in ch if j + 1 <= qpos]
                    j = ch[(t // 8 + t + 2 * h + b) % len(ch)]
                    q[c] = _aimed(K[:qpos + 1, c], K[j, c] + K[j + 1, c] if kind == "pair" else K[j, c])
            cs.add_row(b, qpos + 1, q, [kind] * NH)
    return cs.finish()


# ---------------------------------------------------------------- poisoned pools (GPU tests)
def pages_needed(cs, P):
    """pages poisoned_pool hands out for cs.seqs at page size P"""
    return sum((k.shape[0] + P - 1) // P for k, _ in cs.seqs)


def poisoned_pool(hip, cs, P, dtype, extra_pages=3, seed=0, num_pages=None, candidates=None):
    """a 1-layer pool holding cs.seqs with no clean byte outside the contexts:
    the whole slab 0xFF (a NaN in fp32, bf16 and e4m3fn) before anything is
    written, the slots past a context in its last page NaN, pages handed out
    in a random permutation, table entries past a sequence's pages -1.
    num_pages: the pool's page count (default: the pages the sequences need
    plus extra_pages).  candidates: the page indices the sequences may get
    (default: every page), most wanted first -- the first pages_needed(cs, P)
    of them are permuted and handed out, so a pool far larger than its
    contents (tests/test_gpu_pool_large.py) places them where the caller says.
    Returns (pool, tables (n_seqs, maxp))."""
    L = hip.lib()
    npg = [(k.shape[0] + P - 1) // P for k, _ in cs.seqs]
    if num_pages is None:
        num_pages = sum(npg) + extra_pages
    pool = hip.Pool(1, NH, P, num_pages, dtype=dtype)
    hip.check(L.hpa_memset_async(pool.s.base, 0xFF, pool.s.bytes), "poison")
    hip.check(L.hpa_synchronize())
    if dtype == HPA_FP8:
        pool.set_scales(K_SCALE[None, :], V_SCALE[None, :])
    rng = np.random.default_rng([seed, P, int(dtype)])
    if candidates is None:
        perm = rng.permutation(num_pages).astype(np.int32)
    else:
        cand = np.asarray(candidates, np.int64).reshape(-1)[:sum(npg)]
        assert cand.size == sum(npg) == np.unique(cand).size and cand.min() >= 0 and cand.max() < num_pages
        perm = rng.permutation(cand).astype(np.int32)
    tables = np.full((len(cs.seqs), max(npg)), -1, np.int32)
    nxt = 0
    for si, (k, v) in enumerate(cs.seqs):
        n = npg[si]
        tables[si, :n] = perm[nxt:nxt + n]
        nxt += n
        pad = np.full((n * P - k.shape[0], C), np.nan, np.float32)
        pool.write_tokens(0, tables[si, :n], np.concatenate([k, pad]), np.concatenate([v, pad]))
    return pool, tables


# ---------------------------------------------------------------- engine level (tests/test_gpu_layer_hard.py)
GAMMA = {128: 25.0}  # by C, else 10: at C = 128 the same |q| as 10 gives at C = 768 (q ~ gamma 0.02 sqrt(C))


def peaked_params(cfgd, seed, gamma=None):
    """synth.params with the Q rows of qkvw and qkvb of every layer times gamma (default: GAMMA's for the width)"""
    gamma = GAMMA.get(cfgd["C"], 10.0) if gamma is None else gamma
    p = synth.params(cfgd, seed=seed).copy()
    off, sz = synth.offsets(cfgd), synth.sizes(cfgd)
    C, nl = cfgd["C"], cfgd["L"]
    w = p[off[4]:off[4] + sz[4]].reshape(nl, 3 * C, C)
    b = p[off[5]:off[5] + sz[5]].reshape(nl, 3 * C)
    w[:, :C] *= np.float32(gamma)
    b[:, :C] *= np.float32(gamma)
    return p


def input_conditions(ref, x0, K, V, ctx):
    """(largest softmax weight, E) per (row, head) of layer 0, from float64 alone"""
    q = ref._qkv(np.asarray(x0, np.float64), 0, 0, ref.C)
    B = q.shape[0]
    wmax, E = np.zeros((B, ref.NH)), np.zeros((B, ref.NH))
    for b in range(B):
        for h in range(ref.NH):
            c = slice(h * 64, (h + 1) * 64)
            r = attend(q[b, c], K[b][:ctx[b], c], V[b][:ctx[b], c])
            wmax[b, h], E[b, h] = r.wmax[0], r.E[0]
    return wmax, E
