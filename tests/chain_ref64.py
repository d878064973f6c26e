"""Float64 reference and checker of the bf16-weight decode chain
(hpa_chain_b16.hip: attproj -> fc -> fcproj -> qkv(l+1), and the step's first
launch), one phase at a time and every phase ON THE KERNEL'S OWN INPUT to it.

Numpy only: no GPU, no oracle.  The GPU tests (tests/test_gpu_chain_b16.py) and
the CPU self-test (tests/test_chain_ref64.py, a numpy emulation of the chain
and its mutants) share every check here.

Why per phase: through the engine the chain is held at 4e-3 of max|x| only,
because one bf16 rounding flip in a phase's operand re-rounds part of the next
phase's.  The chain leaves res2, fch, res, q_out and the K/V rows in buffers
the caller owns, so each phase can be recomputed from what the kernel itself
fed it, and the cascade is gone.

Every reference uses the bf16-rounded weights, exact products and float64
sums.  The base bound is the project's (tests/test_gpu_fused.py):

    bound = 4e-6 * sum_k |a_k| |w_nk| + 2e-6

  B  attproj   res2 = res + rb(att) . Wap^T + b_ap within bound.  att is fp32
               in memory, so its rounding is deterministic: no allowance.
  C  fc        a64 = LN2(res2) in float64.  The kernel rounds ITS fp32
               one-pass LayerNorm, so an element may legally round either way
               when a64 is within delta of a rounding boundary:
                 delta = 2^-19 (|g| (|x| + |m|) rstd (2 + (m^2 + v)/(v + eps)) + |b|)
               2^-19 is 32 fp32 ulps: each statistic is a sum about 36 adds
               deep (3 steps x 8 values per lane, 2 shuffles, 8 waves), x - m
               carries the error of m and its own rounding (|x| + |m|), the
               one-pass variance S2/C - m^2 carries the errors of both terms,
               (m^2 + v) relative to v + eps under the root (half of it in
               rstd), and the gain and bias add a rounding each.
               S = {k : rb(a64 - delta) != rb(a64 + delta)}, |S| <= 32 a row.
               pre = rb_lo(a) . Wfc^T + b_fc, flip = sum_{k in S} (rb_hi -
               rb_lo)_k |w_nk|; fch is stored as bf16, |gelu'| <= 1.13:
                 |got - gelu(pre)| <= 1.13 (bound + flip)
                                      + half_ulp_bf16(|gelu(pre)| + 1.13 (bound + flip))
  D  fcproj    res = res2 + fch . Wfp^T + b_fp (K = 3072) within bound; fch
               is exact bf16, nothing to allow for.  last: stats_out[j][row]
               = (sum, sum of squares) of 16-column tile j of the kernel's
               res.  tests/test_gpu_fused.py::test_fused_resid_with_stats
               writes that buffer and asserts nothing about it, so the
               tolerance here is the base bound read for a sum of 16 terms
               (a = x, w = 1, and a = x, w = x): 4e-6 sum|x| + 2e-6 and
               4e-6 sum x^2 + 2e-6.
  E  qkv(l+1)  q and the K/V rows are fp32 (or bf16 K/V), so the rounding of
               the operand is RESOLVED, not allowed for: per row, with S as in
               C, solve got - (rb_lo(a) . W^T + b) ~= D s in the least-squares
               sense (D[:, k] = (rb_hi - rb_lo)_k W[:, k]; every column
               weighted by 1 / its own tolerance, so a bf16 pool's K/V columns,
               noisy by half a bf16 ulp, do not drown the fp32 q columns), set
               s <- clip(round(s), 0, 1), and require all 2304 columns within
               bound (+ half a bf16 ulp of the reference for K/V in a bf16
               pool, as ref64.check_kv).  The kernel's operand row must be a
               legal bf16 rounding of the LayerNorm; nothing else is forgiven.
  first        res == fp32 wte[tok] + wpe[pos] bit for bit, then E.
  padded       rows B .. Mp-1 of res2, fch, res exactly 0.
  placement    over the WHOLE pool, raw storage before against after: the
               changed elements are exactly the K and the V row, every head,
               of (layer + 1, bt[b][pos_b / P], pos_b % P), b < B.  The pool is
               filled with 0xFF bytes first (a NaN in either type), so a
               written element always differs.
  protocol     *err == 0; the counter block after the launch: X1[rb] = NG_B =
               16 (one arrival per attproj unit of the row block), H[rb][p] =
               NG_C / 4 = 8 (the fc units whose 96 columns feed K part p; a
               unit arrives for both row blocks of its group), ticket[quad][g]
               = 4 (one per K part), X2[rb] = NG_D = 16 (the last part of a
               (quad, tile group) arrives for every live row block of the
               quad); every other int of the block 0.  Derived from the
               arrival code of hpa_chain_b16.hip, which is the truth.
  guard        the words after each buffer, q_out rows >= B and stats_out rows
               >= Mp keep their sentinel.

`make_inputs` builds operands OFF the synthetic regime (zero-mean rows, gain
about 1, variance >> eps) that every engine-level test lives in;
`input_conditions` asserts, on float64 values alone, that a phase's LayerNorm
input really is off it.
"""
import numpy as np

from pagedattn import from_bf16_bits, from_frag, from_frag_bf16
from ref64 import _rb, gelu, half_ulp_bf16

C, NH, HS = 768, 12, 64
EPS = 1e-5
NG_B, NG_C, NG_D = 16, 32, 16                     # tile groups per phase (hpa_chain_b16.hip)
K_X1, K_H, K_X2, K_TICK, K_LINES, K_PAD = 0, 16, 80, 96, 160, 32
SENT32 = 0x7FC0BEEF                               # a quiet NaN: "never written"
OUTLIER_COLS = (138, 447)


class ChainMismatch(AssertionError):
    """.check: the name of the check that failed"""

    def __init__(self, check, msg):
        self.check = check
        super().__init__(f"[{check}] {msg}")


def gemm_bound(a, W):
    return 4e-6 * (np.abs(a) @ np.abs(W).T) + 2e-6


def _worst(check, ratio, what):
    """ratio (rows, cols) against 1; returns its maximum"""
    ratio = np.asarray(ratio)
    if ratio.size == 0:
        return 0.0
    w = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("nan")
    if not np.all(ratio <= 1.0):  # a NaN fails
        bad = np.argwhere(~(ratio <= 1.0))
        r, c = (int(t) for t in bad[0])
        raise ChainMismatch(check, f"{what}: {len(bad)} elements over the bound, first (row {r}, column {c}) "
                                   f"at {ratio[r, c]:.3g} of it; worst {w:.3g}")
    return w


def check_padded(name, x, B):
    """rows B.. of the row-major x exactly 0"""
    pad = np.asarray(x)[B:]
    if pad.size and not np.all(pad == 0):
        r, c = (int(t) for t in np.argwhere(pad != 0)[0])
        raise ChainMismatch("padded", f"{name}: padded row {B + r} column {c} holds {pad[r, c]!r}")


# ---------------------------------------------------------------- the LayerNorm interval
def ln_stats(x):
    x = np.asarray(x, np.float64)
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return m, v


def ln_interval(x, g, b):
    """(a64, rb_lo, rb_hi, S) of LN(x) (eps 1e-5): the float64 LayerNorm, the
    bf16 roundings of a64 -/+ delta and the mask where they differ"""
    x = np.asarray(x, np.float64)
    g, b = np.asarray(g, np.float64), np.asarray(b, np.float64)
    m, v = ln_stats(x)
    rstd = 1.0 / np.sqrt(v + EPS)
    a = (x - m) * rstd * g + b
    delta = 2.0 ** -19 * (np.abs(g) * (np.abs(x) + np.abs(m)) * rstd * (2 + (m * m + v) / (v + EPS)) + np.abs(b))
    lo, hi = _rb(a - delta), _rb(a + delta)
    return a, lo, hi, lo != hi


def check_S(S, where):
    n = S.sum(-1)
    if n.size and n.max() > 32:
        raise ChainMismatch("S", f"{where}: row {int(n.argmax())} has {int(n.max())} ambiguous elements (> 32)")
    return int(n.max()) if n.size else 0


# ---------------------------------------------------------------- the phases
def check_attproj(att, res_in, res2, Wap, b_ap, B):
    """row-major fp32 (Mp, C) att / res_in / res2; Wap (C, C) float64 bf16 values"""
    a = _rb(att[:B])
    ref = res_in[:B].astype(np.float64) + a @ Wap.T + np.asarray(b_ap, np.float64)
    r = _worst("B", np.abs(res2[:B].astype(np.float64) - ref) / gemm_bound(a, Wap), "res2 = res + att.Wap^T + b")
    check_padded("res2", res2, B)
    return r


def fch_values(fch_bits, Mp):
    """the chain's fch buffer (bf16 frag layout, uint16) -> (Mp, 4C) float64"""
    return from_bf16_bits(from_frag_bf16(fch_bits, Mp, 4 * C)).astype(np.float64)


def check_fc(res2, fch_bits, ln2_w, ln2_b, Wfc, b_fc, B):
    """res2 row-major (Mp, C) fp32 (the kernel's), fch_bits the raw buffer.
    Returns (worst ratio, max |S|)"""
    Mp = res2.shape[0]
    _, lo, hi, S = ln_interval(res2[:B], ln2_w, ln2_b)
    nS = check_S(S, "LN2(res2)")
    pre = lo @ Wfc.T + np.asarray(b_fc, np.float64)
    slack = 1.13 * (gemm_bound(lo, Wfc) + ((hi - lo) * S) @ np.abs(Wfc).T)
    ref = gelu(pre)
    got = fch_values(fch_bits, Mp)
    # the same inequality, reported as what is left of the error beyond the store's half ulp, over the slack
    r = _worst("C", np.maximum(np.abs(got[:B] - ref) - half_ulp_bf16(np.abs(ref) + slack), 0.0) / slack,
               "fch = gelu(LN2(res2).Wfc^T + b)")
    check_padded("fch", got, B)
    return r, nS


def check_fcproj(res2, fch_bits, res, Wfp, b_fp, B):
    Mp = res2.shape[0]
    a = fch_values(fch_bits, Mp)[:B]
    ref = res2[:B].astype(np.float64) + a @ Wfp.T + np.asarray(b_fp, np.float64)
    r = _worst("D", np.abs(res[:B].astype(np.float64) - ref) / gemm_bound(a, Wfp), "res = res2 + fch.Wfp^T + b")
    check_padded("res", res, B)
    return r


def check_stats(res, stats, stats_mp):
    """stats flat fp32 [C/16][stats_mp][2] against the tiles of the kernel's res (Mp, C)"""
    Mp = res.shape[0]
    st = np.asarray(stats, np.float32).reshape(C // 16, stats_mp, 2)
    x = res.astype(np.float64).reshape(Mp, C // 16, 16).transpose(1, 0, 2)  # (tile, row, 16)
    r1 = np.abs(st[:, :Mp, 0] - x.sum(-1)) / (4e-6 * np.abs(x).sum(-1) + 2e-6)
    r2 = np.abs(st[:, :Mp, 1] - (x * x).sum(-1)) / (4e-6 * (x * x).sum(-1) + 2e-6)
    r = max(_worst("stats", r1, "LNf partial sums"), _worst("stats", r2, "LNf partial sums of squares"))
    rest = st[:, Mp:].view(np.uint32)
    if rest.size and not np.all(rest == SENT32):
        raise ChainMismatch("guard", "stats_out written at a row >= Mp")
    return r


def check_qkv(res, ln1_w, ln1_b, Wqkv, b_qkv, q, k, v, kv_bf16, B):
    """res (Mp, C) the kernel's; q, k, v (B, C) fp32 values as stored.
    Returns (worst ratio to the bound, max |S|)"""
    _, lo, hi, S = ln_interval(res[:B], ln1_w, ln1_b)
    nS = check_S(S, "LN1(res)")
    got = np.concatenate([q[:B], k[:B], v[:B]], 1).astype(np.float64)
    ref0 = lo @ Wqkv.T + np.asarray(b_qkv, np.float64)
    bnd = gemm_bound(lo, Wqkv)
    kvcol = np.arange(3 * C) >= C
    ratio = np.zeros_like(got)
    for r in range(B):
        idx = np.nonzero(S[r])[0]
        fit = ref0[r]
        if len(idx):
            D = (hi[r, idx] - lo[r, idx]) * Wqkv[:, idx]
            w = 1.0 / (bnd[r] + (half_ulp_bf16(ref0[r]) * kvcol if kv_bf16 else 0.0))
            rhs = np.nan_to_num(got[r] - ref0[r], nan=0.0, posinf=0.0, neginf=0.0)
            s = np.linalg.lstsq(D * w[:, None], rhs * w, rcond=None)[0]
            fit = ref0[r] + D @ np.clip(np.round(s), 0, 1)
        d = np.abs(got[r] - fit)
        if kv_bf16:
            d = np.where(kvcol, np.maximum(d - half_ulp_bf16(fit), 0.0), d)
        ratio[r] = d / bnd[r]
    return _worst("E", ratio, "q | K | V = LN1(res).Wqkv^T + b"), nS


def check_embed(res, wte, wpe, tok, pos, B):
    want = (wte[np.asarray(tok[:B])] + wpe[np.asarray(pos[:B])]).astype(np.float32)
    if not np.array_equal(res[:B].view(np.uint32), want.view(np.uint32)):
        r, c = (int(t) for t in np.argwhere(res[:B].view(np.uint32) != want.view(np.uint32))[0])
        raise ChainMismatch("embed", f"res row {r} column {c}: {res[r, c]!r}, wte + wpe gives {want[r, c]!r}")
    check_padded("res", res, B)


# ---------------------------------------------------------------- the pool
def pool_geom(L, pages, P, bf16):
    pe = 2 * NH * P * HS
    return dict(L=L, pages=pages, P=P, bf16=bool(bf16), ch=8 if bf16 else 4, page_elems=pe, layer_elems=pages * pe)


def kv_index(geom, layer, page, slot):
    """(K, V) storage element indices, (.., C) each, of the rows (page, slot) of `layer`
    (include/hip_paged_attn.h: K tile [64/ch][P][ch], V tile [P][64] per head)"""
    P, ch = geom["P"], geom["ch"]
    page = np.asarray(page, np.int64)[..., None]
    slot = np.asarray(slot, np.int64)[..., None]
    c = np.arange(C)
    h, d = c // HS, c % HS
    base = layer * geom["layer_elems"] + page * geom["page_elems"]
    return (base + h * (P * HS) + ((d // ch) * P + slot) * ch + d % ch,
            base + (NH + h) * (P * HS) + slot * HS + d)


def _where_in_pool(geom, i):
    l, r = divmod(int(i), geom["layer_elems"])
    pg, r = divmod(r, geom["page_elems"])
    t, r = divmod(r, geom["P"] * HS)
    return f"layer {l} page {pg} {'KV'[t // NH]} head {t % NH} tile element {r}"


def pool_values(geom, img, idx):
    x = np.asarray(img)[idx]
    return from_bf16_bits(x) if geom["bf16"] else x.view(np.float32)


def check_placement(geom, before, after, layer, bt, pos, B):
    """before / after: the pool's whole storage (uint16 or uint32, flat).  layer:
    the layer written, None when nothing may be.  Returns (k, v) (B, C) fp32 as stored"""
    changed = np.nonzero(np.asarray(before) != np.asarray(after))[0]
    if layer is None:
        if len(changed):
            raise ChainMismatch("placement", f"pool written by a launch without a qkv phase: "
                                             f"{_where_in_pool(geom, changed[0])}")
        return None, None
    P = geom["P"]
    pos = np.asarray(pos[:B], np.int64)
    page = np.asarray(bt)[np.arange(B), pos // P]
    assert (page >= 0).all() and (page < geom["pages"]).all(), "the test's own block table"
    ki, vi = kv_index(geom, layer, page, pos % P)
    want = np.sort(np.concatenate([ki.ravel(), vi.ravel()]))
    assert len(np.unique(want)) == len(want), "two sequences share a slot: the test's own block table"
    stray = np.setdiff1d(changed, want)
    if len(stray):
        raise ChainMismatch("placement", f"{len(stray)} elements written outside the {B} appended rows, first "
                                         f"{_where_in_pool(geom, stray[0])}")
    miss = np.setdiff1d(want, changed)
    if len(miss):
        raise ChainMismatch("placement", f"{len(miss)} elements of the appended rows not written, first "
                                         f"{_where_in_pool(geom, miss[0])}")
    return pool_values(geom, after, ki), pool_values(geom, after, vi)


# ---------------------------------------------------------------- protocol and guards
def expected_counters(B, first=False):
    """the counter block (K_LINES lines of K_PAD ints) a launch on zeroed counters leaves"""
    c = np.zeros(K_LINES * K_PAD, np.int32)
    if first:
        return c
    R = (B + 15) // 16
    for rb in range(R):
        c[(K_X1 + rb) * K_PAD] = NG_B
        c[(K_X2 + rb) * K_PAD] = NG_D
        for p in range(4):
            c[(K_H + rb * 4 + p) * K_PAD] = NG_C // 4
    for quad in range((R + 3) // 4):
        for g in range(NG_D):
            c[(K_TICK + quad * NG_D + g) * K_PAD] = 4
    return c


def _line_name(line):
    if line < K_H:
        return f"X1[{line}]"
    if line < K_X2:
        return f"H[{(line - K_H) // 4}][{(line - K_H) % 4}]"
    if line < K_TICK:
        return f"X2[{line - K_X2}]"
    return f"ticket[{(line - K_TICK) // NG_D}][{(line - K_TICK) % NG_D}]"


def check_protocol(ctr, err, B, first=False):
    if int(err) != 0:
        raise ChainMismatch("protocol", f"*err = {int(err)} after the launch")
    want = expected_counters(B, first)
    ctr = np.asarray(ctr, np.int32)
    assert ctr.shape == want.shape
    bad = np.nonzero(ctr != want)[0]
    if len(bad):
        i = int(bad[0])
        raise ChainMismatch("protocol", f"counter {_line_name(i // K_PAD)} int {i % K_PAD}: {int(ctr[i])}, "
                                        f"expected {int(want[i])} ({len(bad)} ints differ)")


def check_guards(guards):
    """guards: name -> (array of words that must still hold their fill, fill)"""
    for name, (words, fill) in guards.items():
        words = np.asarray(words)
        if words.size and not np.all(words == fill):
            i = int(np.nonzero(words.ravel() != fill)[0][0])
            raise ChainMismatch("guard", f"{name}: word {i} overwritten with {int(words.ravel()[i]):#x}")


# ---------------------------------------------------------------- inputs off the synthetic regime
def input_conditions(x, g, b, name=""):
    """x (rows, C) float64: the LayerNorm input of a phase.  Asserts it is off the
    synthetic regime (quarters and eighths of the rows, rounded down); returns max |S|"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    m, v = ln_stats(x)
    sd = np.sqrt(v)
    off = int((np.abs(m) / sd >= 0.5).sum())
    low = int(((v / EPS >= 0.2) & (v / EPS <= 20)).sum())
    out = int((np.abs(x) > 20 * sd).any(-1).sum())
    assert off >= n // 4, f"{name}: {off} of {n} rows with |mean| >= 0.5 sd"
    assert low >= n // 8, f"{name}: {low} of {n} rows with variance within [0.2, 20] eps"
    assert out >= n // 4, f"{name}: {out} of {n} rows with an element beyond 20 sd"
    g, b = np.asarray(g), np.asarray(b)
    assert g.min() <= np.float32(0.05) and g.max() >= 2.0, f"{name}: LayerNorm gain spans [{g.min()}, {g.max()}]"
    assert b.min() <= -1.0 and b.max() >= 1.0, f"{name}: LayerNorm bias spans [{b.min()}, {b.max()}]"
    S = ln_interval(x, g, b)[3]
    assert S.sum(-1).max() <= 32, f"{name}: {S.sum(-1).max()} ambiguous elements in a row"
    return int(S.sum(-1).max())


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def regime_rows(rng, n, scale=0.5):
    """(n, C) fp32 rows by kind = row % 8: 3 small (sd 0.005, no offset: variance
    about 2.5 eps); 1, 2, 5, 7 carry one element of +-30 in column 138 or 447 (beyond
    20 sd; their sd about 1.2) and an offset of +-U(0.65, 0.85); 0, 4, 6 an offset of
    +-U(0.32, 0.42): |mean| between 0.5 and 0.75 sd once attproj's product is added,
    where the one-pass variance has lost a bit and the interval's (m^2 + v) / (v + eps)
    term is felt, yet |S| stays <= 32"""
    x = scale * rng.standard_normal((n, C))
    for r in range(n):
        kind = r % 8
        sign = 1 if rng.uniform() < 0.5 else -1
        if kind == 3:
            x[r] = 0.005 * rng.standard_normal(C)
        elif kind in (1, 2, 5, 7):
            x[r] += sign * rng.uniform(0.65, 0.85)
            x[r, OUTLIER_COLS[kind & 1]] = 30.0 * (1 if r % 3 else -1)
        else:
            x[r] += sign * rng.uniform(0.32, 0.42)
    return _f32(x)


def small_row(r):
    return r % 8 == 3


def _ln_params(rng):
    g = rng.uniform(0.05, 2.0, C)
    b = rng.uniform(-1.0, 1.0, C)
    g[[11, 500]], g[[12, 501]] = 0.05, 2.0
    b[[13, 502]], b[[14, 503]] = -1.0, 1.0
    return _f32(g), _f32(b)


# att rounding edges, in row 0 of every row block (a plain row): (column, value)
def _edges():
    f = np.float32
    mid_e, mid_o = f(4.0 + 2.0 ** -6), f(4.0 + 2.0 ** -5 + 2.0 ** -6)  # ties: lower neighbour 0x4080 even, 0x4081 odd
    return [(5, mid_e), (70, -mid_e), (201, mid_o), (333, -mid_o),
            (402, mid_e), (470, mid_o), (533, -mid_e),
            (600, np.nextafter(mid_e, f(0))), (611, np.nextafter(mid_e, f(8))),
            (650, -np.nextafter(mid_o, f(0))), (661, -np.nextafter(mid_o, f(8))),
            (700, f(0.0)), (701, f(-0.0)), (766, f(2.0 ** -126)), (767, -f(2.0 ** -126))]


_BASE = {}


def _base_inputs(seed, V, maxT):
    """everything of make_inputs that does not depend on B: the weights, and 256 rows of
    res / att / tokens of which a batch takes the first B (so a row of a small batch has
    the same inputs inside a larger one)"""
    key = (seed, V, maxT)
    if key in _BASE:
        return _BASE[key]
    rng = np.random.default_rng(seed)
    u = lambda s, *shape: _f32(rng.uniform(-s, s, shape))
    d = dict(V=V, maxT=maxT)
    d["w_ap"], d["w_fc"], d["w_qkv"] = u(0.035, C, C), u(0.035, 4 * C, C), u(0.035, 3 * C, C)
    d["w_fp"] = u(0.0005, C, 4 * C)
    d["b_ap"], d["b_fp"], d["b_fc"], d["b_qkv"] = u(0.002, C), u(0.002, C), u(0.1, 4 * C), u(0.1, 3 * C)
    for n in range(3, 4 * C, 7):
        s = n % 24
        row = np.zeros(C, np.float32)
        row[32 * s:32 * s + 32] = u(0.2, 32)
        d["w_fc"][n] = row
        d["b_fc"][n] = np.float32(rng.uniform(-3.2, -1.2))
    d["ln2_w"], d["ln2_b"] = _ln_params(rng)
    d["ln1_w"], d["ln1_b"] = _ln_params(rng)
    # the first launch: token rows by regime_rows, position rows tiny (the row keeps its token's regime)
    d["wte"] = regime_rows(rng, V)
    d["wpe"] = u(0.002, maxT, C)
    d["res"] = regime_rows(rng, 256)
    att = _f32(0.5 * rng.standard_normal((256, C)))
    for r in range(256):
        if small_row(r):
            att[r] *= 0.01
        if r % 16 == 0:
            for col, val in _edges():
                att[r, col] = val
    d["att"] = att
    tok = (np.arange(256) * 9 + 1) % V
    tok[0], tok[1] = 0, V - 1
    d["tokens"] = tok.astype(np.int32)
    d["W64"] = {k: _rb(d[k]) for k in ("w_ap", "w_fc", "w_fp", "w_qkv")}
    _BASE[key] = d
    return d


def make_inputs(B, seed, V=320, maxT=200):
    """operands of one chain launch and one first launch at B rows, as fp32 numpy
    arrays (weights unrounded; W64[name]: their bf16 values in float64); res and
    att (Mp, C) with zero padded rows.  The same seed gives the same weights at
    every B, and a smaller batch the first rows of a larger one.

    res rows by regime_rows; att rows 0.5 N(0, 1), the small rows' att small too,
    so res2 = res + att.Wap^T + b keeps the regime (Wap, Wfc, Wqkv U(-0.035,
    0.035); b_ap, b_fp U(-0.002, 0.002)).  fcproj adds fch.Wfp^T, whose rows are
    O(1) . |Wfp| sqrt(3072) whatever the row's scale (LN2 normalises it), so Wfp
    is U(-0.0005, 0.0005): the product stays near the small rows' sd and res (LN1's
    input) keeps the regime as well.  The bound scales with |w|, so phase D is
    held as tightly relative to its product as with larger weights.
    Every 7th fc column (n % 7 == 3) reads one 32-deep k-step only (weights
    U(-0.2, 0.2)) under a bias from U(-3.2, -1.2): almost never touched by an
    ambiguous LN2 element (flip = 0), and where the tanh and erf forms of GELU
    differ by many bf16 ulps of the (small) result."""
    assert 1 <= B <= 256
    base = _base_inputs(seed, V, maxT)
    Mp = (B + 15) // 16 * 16
    d = dict(base, B=B, Mp=Mp)
    for k in ("res", "att"):
        x = np.zeros((Mp, C), np.float32)
        x[:B] = base[k][:B]
        d[k] = x
    d["tokens"] = base["tokens"][:B].copy()
    return d


def make_paging(B, P, F=None, free=16, per_seq=4, seed=0):
    """block table (B, per_seq + 3) with unused entries -1 and permuted page ids,
    ragged positions on a fill of F = 3 P (ref64.ragged_positions), `free` pages
    that no sequence owns.  At P = 8 the fill is 3 P + 1: on 24 the generator
    steps by 7 modulo 21 and gives rows 16..31 three slots only, which
    check_position_mix refuses; modulo 22 it visits every residue"""
    from ref64 import check_position_mix, ragged_positions
    F = (3 * P + (P == 8)) if F is None else F
    pos = ragged_positions(B, P, F)
    check_position_mix(pos, P)
    pages = B * per_seq + free
    perm = np.random.default_rng(1000 + seed).permutation(pages)
    bt = np.full((B, per_seq + 3), -1, np.int32)
    bt[:, :per_seq] = perm[:B * per_seq].reshape(B, per_seq)
    assert pos.max() // P < per_seq
    return dict(P=P, pos=pos.astype(np.int32), bt=bt, pages=pages, free_pages=perm[B * per_seq:].copy())


# ---------------------------------------------------------------- one launch, every check
def check_launch(inp, pg, geom, out, last=0, first=False, layer=0, collect=False):
    """out: what a launch left -- res2 / res (fp32 frag flat, Mp x C), fch (uint16
    flat), q (Mp, C) fp32 with SENT32 below row B, pool_before / pool_after, ctr,
    err, stats (flat or None), stats_mp, guards; first: res, q, pool, zero (the
    zeroed block with its tail, uint32) and zero_words.
    Returns (ratios, failures); raises the first ChainMismatch unless collect"""
    B, Mp, W = inp["B"], inp["Mp"], inp["W64"]
    ratios, failures = {}, {}

    def run(name, fn):
        try:
            fn()
        except ChainMismatch as e:
            if not collect:
                raise
            failures.setdefault(e.check, str(e))

    res = from_frag(np.asarray(out["res"], np.float32), Mp, C)
    kv = {}

    def placement():
        kv["k"], kv["v"] = check_placement(geom, out["pool_before"], out["pool_after"],
                                           None if last else layer + 1, pg["bt"], pg["pos"], B)

    def phase_e():
        if last or "k" not in kv:
            return
        ratios["E"], ratios["S1"] = check_qkv(res, inp["ln1_w"], inp["ln1_b"], W["w_qkv"], inp["b_qkv"],
                                              out["q"], kv["k"], kv["v"], geom["bf16"], B)

    def q_guard():
        rows = out["q"][0 if last else B:].view(np.uint32)
        check_guards({"q_out rows that must stay": (rows, SENT32)})

    if first:
        run("embed", lambda: check_embed(res, inp["wte"], inp["wpe"], inp["tokens"], pg["pos"], B))
        z = np.asarray(out["zero"], np.uint32)
        n = out["zero_words"]
        run("protocol", lambda: check_guards({"zero tail": (z[n:], 0xFFFFFFFF)}))

        def zeroed():
            if not np.all(z[:n] == 0):
                raise ChainMismatch("protocol", f"zero block: word {int(np.nonzero(z[:n])[0][0])} not zeroed")
        run("protocol", zeroed)
    else:
        res2 = from_frag(np.asarray(out["res2"], np.float32), Mp, C)
        run("B", lambda: ratios.__setitem__("B", check_attproj(inp["att"], inp["res"], res2, W["w_ap"],
                                                               inp["b_ap"], B)))

        def phase_c():
            ratios["C"], ratios["S2"] = check_fc(res2, out["fch"], inp["ln2_w"], inp["ln2_b"], W["w_fc"],
                                                 inp["b_fc"], B)
        run("C", phase_c)
        run("D", lambda: ratios.__setitem__("D", check_fcproj(res2, out["fch"], res, W["w_fp"], inp["b_fp"], B)))
        if out.get("stats") is not None:
            run("stats", lambda: ratios.__setitem__("stats", check_stats(res, out["stats"], out["stats_mp"])))
        run("protocol", lambda: check_protocol(out["ctr"], out["err"], B))
    run("placement", placement)
    run("E", phase_e)
    run("guard", q_guard)
    run("guard", lambda: check_guards(out.get("guards", {})))
    return ratios, failures
