"""A plain float64 reference of one decode layer, and the K/V-append checker.

Numpy only: no oracle, no GPU.  `Ref64` restates one transformer layer of the
decode path in float64 (exact sums, for all practical purposes) from the 16
checkpoint tensors (synth.offsets):

  ln(x, w, b)              LayerNorm, eps 1e-5, population variance
  kv_rows(x_l, l)          the K/V rows a decode step appends at layer l:
                           columns C..3C of LN1(x_l) @ qkvw[l].T + qkvb[l]
  layer_out(x_l, l, K, V, ctx)
                           per-head softmax(q.k / 8) over keys 0..ctx-1, .V,
                           attproj + residual, LN2, fc, the tanh GELU of
                           hpa::gelu_ref, fcproj + residual

With w_bf16 it restates the oracle's bf16-weights rule
(oracle/paged_oracle.c, oracle_paged_set_w_bf16 / round_bf16_n): the four
layer matrices are rounded to bf16 (nearest even), every GEMM's A operand
(LN1 out, attention out, LN2 out, GELU out) is rounded to bf16 first, biases
stay fp32, and the sums are exact.  With kv_bf16 the rows kv_rows returns are
pagedattn.round_bf16 of the fp32-rounded values (what a bf16 pool stores);
kv_rows_exact returns the unrounded float64 rows the tolerance is taken from.

`check_kv` is the checker the GPU tests (tests/test_gpu_kv_append.py) and the
CPU self-test (tests/test_kv_ref64.py) share.  Per layer and sequence it takes
the K/V rows before and after some steps, the interval [pos, pos + n) the
steps must have written, and the float64 rows where they are known, and holds:

  (a) every row outside the interval is bit-identical to `before`;
  (b) every (row, head) inside it differs from `before`;
  (c) every row inside it equals its reference:
          |got - ref| <= rtol * max|ref row|  (+ half a bf16 ulp of ref for
          a bf16 pool, the store's rounding).

The half ulp is the exact one, 2^(floor(log2 |ref|) - 8): between 2^-9 |ref|
(mantissa just under 2) and 2^-8 |ref| (mantissa 1).  A flat 2^-9 |ref| would
refuse a correctly rounded store of any value whose mantissa is below 1.5.

Rows of pages that no sequence owns cannot be read through the model API, so
a stray store into a free page is outside what this checker sees.
"""
import numpy as np

from pagedattn import round_bf16
from synth import offsets, sizes

HS = 64  # head size of every model the engine runs
GELU_S = float(np.array([0x3F4C4229], np.uint32).view(np.float32)[0])  # sqrtf(2/pi), hpa::gelu_ref
GELU_C = float(np.float32(0.044715))


def _rb(a):
    """float64 -> the float64 value of its bf16 rounding (through fp32, as the engine's operands are)"""
    return round_bf16(np.asarray(a, np.float64).astype(np.float32)).astype(np.float64)


def ln(x, w, b):
    """LayerNorm over the last axis: eps 1e-5, population variance"""
    x = np.asarray(x, np.float64)
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + 1e-5) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def gelu(x):
    return 0.5 * x * (1.0 + np.tanh(GELU_S * (x + GELU_C * x * x * x)))


def half_ulp_bf16(ref):
    """half a bf16 ulp (8 significant bits) of every element of ref"""
    a = np.abs(np.asarray(ref, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, np.exp2(e - 8), 0.0)


class Ref64:
    def __init__(self, cfgd, params, w_bf16=False, kv_bf16=False):
        self.cfg = cfgd
        self.C, self.NH, self.L = cfgd["C"], cfgd["NH"], cfgd["L"]
        assert self.C == self.NH * HS
        self.w_bf16, self.kv_bf16 = bool(w_bf16), bool(kv_bf16)
        self.p = np.asarray(params, np.float32)
        self.off, self.sz = offsets(cfgd), sizes(cfgd)
        C = self.C
        self.wte = self._t(0).reshape(cfgd["V"], C)
        self.wpe = self._t(1).reshape(cfgd["maxT"], C)

    def _t(self, i):
        return self.p[self.off[i]:self.off[i] + self.sz[i]]

    def _layer(self, i, l, shape):
        n = self.sz[i] // self.L
        return self._t(i)[l * n:(l + 1) * n].reshape(shape)

    def _mat(self, i, l, shape):
        """layer matrix (OC, C) as float64, bf16-rounded under w_bf16"""
        w = self._layer(i, l, shape)
        return (round_bf16(w) if self.w_bf16 else w).astype(np.float64)

    def _a(self, x):
        """a GEMM's A operand"""
        return _rb(x) if self.w_bf16 else x

    def embed(self, tok, pos):
        """fp32 wte[tok] + wpe[pos], the engine's exact embedding add"""
        return self.wte[np.asarray(tok)] + self.wpe[np.asarray(pos)]

    def _qkv(self, x, l, lo, hi):
        C = self.C
        a = self._a(ln(x, self._layer(2, l, C), self._layer(3, l, C)))
        w = self._mat(4, l, (3 * C, C))[lo:hi]
        return a @ w.T + self._layer(5, l, 3 * C)[lo:hi].astype(np.float64)

    def kv_rows_exact(self, x, l):
        """(k, v) float64, unrounded; x (C,) or (B, C)"""
        C = self.C
        kv = self._qkv(x, l, C, 3 * C)
        return kv[..., :C], kv[..., C:]

    def kv_rows(self, x, l):
        """(k, v) float64: what the pool holds (bf16-rounded under kv_bf16)"""
        k, v = self.kv_rows_exact(x, l)
        if self.kv_bf16:
            return _rb(k), _rb(v)
        return k, v

    def _attend(self, q, K, V, ctx):
        NH = self.NH
        q = q.reshape(NH, HS)
        K = np.asarray(K[:ctx], np.float64).reshape(ctx, NH, HS)
        V = np.asarray(V[:ctx], np.float64).reshape(ctx, NH, HS)
        s = np.einsum("hd,thd->ht", q, K) / 8.0
        s = np.exp(s - s.max(-1, keepdims=True))
        s /= s.sum(-1, keepdims=True)
        return np.einsum("ht,thd->hd", s, V).reshape(NH * HS)

    def layer_out(self, x, l, K, V, ctx):
        """the layer's output row(s).  x (C,), K/V (>= ctx, C), ctx int -- or
        x (B, C) with K/V sequences of B arrays and ctx of B ints.  K/V hold
        the keys of positions 0..ctx-1, the row appended by this step included."""
        C = self.C
        x = np.asarray(x, np.float64)
        if x.ndim == 1:
            return self.layer_out(x[None], l, [K], [V], [ctx])[0]
        q = self._qkv(x, l, 0, C)
        att = np.stack([self._attend(q[b], K[b], V[b], int(ctx[b])) for b in range(x.shape[0])])
        r2 = x + self._a(att) @ self._mat(6, l, (C, C)).T + self._layer(7, l, C).astype(np.float64)
        h = self._a(ln(r2, self._layer(8, l, C), self._layer(9, l, C)))
        h = h @ self._mat(10, l, (4 * C, C)).T + self._layer(11, l, 4 * C).astype(np.float64)
        h = self._a(gelu(h))
        return r2 + h @ self._mat(12, l, (C, 4 * C)).T + self._layer(13, l, C).astype(np.float64)


# ---------------------------------------------------------------- positions of the ragged cases
def ragged_positions(B, P, F):
    """per-sequence start positions of a ragged case on a pool filled to F:
    0, P-1 (the next step opens page 1), P, F-3, F (as the fill left it), then
    (7 b + 3 (b // 16)) % (F - 3)"""
    special = [0, P - 1, P, F - 3, F]
    return np.array([special[b] if b < len(special) else (7 * b + 3 * (b // 16)) % (F - 3) for b in range(B)],
                    np.int32)


def check_position_mix(pos, P):
    """at least 4 distinct pos % P in every 16-row block of 6 or more rows, and
    min(rows, 3) in a shorter one (0, P and F share a residue, so a batch of 5
    cannot have 4; a one-row block has one)"""
    pos = np.asarray(pos)
    for r0 in range(0, len(pos), 16):
        blk = pos[r0:r0 + 16]
        need = 4 if len(blk) >= 6 else min(len(blk), 3)
        got = len(set(int(p) % P for p in blk))
        assert got >= need, f"rows {r0}..{r0 + len(blk) - 1}: {got} distinct pos % {P}, need {need}"


# ---------------------------------------------------------------- the checker
class KVMismatch(AssertionError):
    """.faults: every violation as (layer, seq, position, head, 'K'|'V', kind, detail),
    kind 'stray' (a), 'unwritten' (b) or 'value' (c); sorted, the first one is the message"""

    def __init__(self, faults):
        self.faults = sorted(faults, key=lambda f: f[:5])
        l, b, t, h, w, kind, detail = self.faults[0]
        super().__init__(f"{kind}: layer {l} sequence {b} position {t} head {h} {w}: {detail}"
                         f" ({len(self.faults)} violations in all)")


def check_kv(before, after, pos, n, ref=None, rtol=0.0, kv_bf16=False, layers=None):
    """before[l][b], after[l][b]: (K, V) float32 arrays (rows, C) of sequence b
    at layer l; `before` may have fewer rows than `after` (rows it lacks are
    unknown: (a) and (b) skip them).  The steps must have written positions
    [pos[b], pos[b] + n[b]).  ref (optional): ref[l][b] = (K, V) float64
    (n[b], C), NaN rows where unknown; ref[l] may be None.
    Raises KVMismatch; returns the worst (c) ratio
    max(0, |got - ref| - bf16 half ulp) / max|ref row|."""
    faults = []
    worst = 0.0
    L = len(after)
    for l in (range(L) if layers is None else layers):
        for b in range(len(after[l])):
            lo, hi = int(pos[b]), int(pos[b]) + int(n[b])
            for wi, w in enumerate("KV"):
                a = np.ascontiguousarray(after[l][b][wi], np.float32)
                bf = np.ascontiguousarray(before[l][b][wi], np.float32)
                rows, C = a.shape
                NH = C // HS
                assert hi <= rows, (l, b, hi, rows)
                known = min(rows, bf.shape[0])
                same = (a[:known].view(np.uint32) == bf[:known].view(np.uint32)).reshape(known, NH, HS)
                same_head = same.all(-1)  # (known, NH)
                ts = np.arange(known)
                inside = (ts >= lo) & (ts < hi)
                for t, h in zip(*np.nonzero(np.where(inside[:, None], same_head, ~same_head))):
                    t, h = int(t), int(h)
                    if inside[t]:
                        faults.append((l, b, t, h, w, "unwritten", "equals the row before the steps"))
                    else:
                        i = int(np.nonzero(~same[t, h])[0][0])
                        faults.append((l, b, t, h, w, "stray",
                                       f"element {i}: {bf[t, h * HS + i]!r} -> {a[t, h * HS + i]!r}"))
                if ref is None or ref[l] is None or hi == lo:
                    continue
                r = np.asarray(ref[l][b][wi], np.float64)
                assert r.shape == (hi - lo, C), (r.shape, hi - lo, C)
                for t in range(lo, hi):
                    rr = r[t - lo]
                    if np.isnan(rr).any():
                        continue
                    scale = float(np.abs(rr).max())
                    d = np.abs(a[t].astype(np.float64) - rr)
                    if kv_bf16:
                        d = np.maximum(d - half_ulp_bf16(rr), 0.0)
                    ratio = d / scale
                    worst = max(worst, float(ratio.max()))
                    bad = (ratio > rtol).reshape(NH, HS)
                    for h in np.nonzero(bad.any(-1))[0]:
                        i = int(np.argmax(ratio.reshape(NH, HS)[h]))
                        faults.append((l, b, t, int(h), w, "value",
                                       f"element {i}: got {a[t, h * HS + i]!r}, reference {rr[h * HS + i]!r}, "
                                       f"ratio {ratio[h * HS + i]:.2e} > {rtol:.2e}"))
    if faults:
        raise KVMismatch(faults)
    return worst
