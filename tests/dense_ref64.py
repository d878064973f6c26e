"""The dense ragged pass (dec_prefill_rows / dec_prefill_layers: prefill,
prefill_ragged, score, score_top, verify) against float64, layer by layer, on
the pass's own inputs.  Numpy only; builds on ref64.Ref64 and ref64.check_kv.

A pass has B sequences; sequence b feeds lens[b] >= 0 rows from position
pos[b]; the R = sum(lens) rows are packed in sequence order.  From the traced
residual stream xs (L+1, R, C) (Model.trace_next_pass: xs[0] after the
embedding, xs[l + 1] after layer l) and the pool's rows of every layer and
sequence before and after the pass, `check_pass` holds:

  embedding   xs[0][r] == wte[tok[r]] + wpe[pos_b + t], bit for bit
  kv          ref64.check_kv over every layer: rows outside [pos, pos + len)
              bit-identical ("stray"), every (row, head) inside changed
              ("unwritten"), every row inside equal to
              ref.kv_rows_exact(xs[l][rows of b], l) ("value"; skipped with
              kv_values=False, an fp8 pool).  A length-0 sequence has an empty
              interval: all of its rows must be bit-identical.
  layer       xs[l + 1][r] against ref.layer_out(xs[l][r], l, K_b, V_b,
              pos_b + t + 1), K_b / V_b the pool's own rows after the pass and
              the causal mask the ctx argument; per row, relative to
              max|xs[l + 1]|
  decode      for every sequence with rows: the engine's logits row against
              float64 LNf(xs[L][last row of b]) @ wte.T within the fused GEMM's
              bound (gemm_bounds: 4e-6 sum|a||w| + 2e-6; bf16 weights: the
              bf16-rounded operands and the midpoint term); the returned next
              id equals the first argmax of that row of the engine's own logits
  score       every row's log-probability against score_ref64.logprob64 of the
              float64 logits from xs[L] within 2 eps_r + kernel_bound, eps_r
              the row's largest logit bound (a sup-norm logit error of eps moves
              the target's logit and the log-sum-exp by at most eps each);
              top_ids exact where the float64 top-2 margin exceeds 2 eps_r;
              score_top alternatives (the pass's own logits rows cannot be read
              from outside, so float64 stands in): rank j's id equals top_ref64's where the
              float64 value at rank j is more than 2 eps_r from both
              neighbours, every returned log-probability within 2 eps_r +
              top_ref64.bound of the float64 one at the returned id, and each
              row's values descending.

`check_pass` returns the worst ratio of every check (value / bar, except "kv"
and "layer", which are the raw ratios the project's tables record) and raises
DenseMismatch naming the checks that failed; with collect=True it returns
(ratios, failures) instead.

`ragged_case`, `prefill_case` and `verify_case` are the lens / pos tables of
tests/test_gpu_dense_pass.py; tests/test_dense_ref64.py asserts their input
conditions (`case_conditions`) from the tables alone.
"""
import numpy as np

import gemm_bounds as gb
import ref64
import score_ref64 as sr
import top_ref64 as tr
from ref64 import ln

F = 96          # fill_random context
MAX_CTX = 160
CHECKS = ("embedding", "kv", "layer", "decode", "score")


class DenseMismatch(AssertionError):
    """.failures: {check: exception}; a "layer" / "score" / "decode" exception carries
    .rows (packed rows or sequences over the bar), a "kv" one is ref64.KVMismatch"""

    def __init__(self, failures):
        self.failures = failures
        super().__init__("; ".join(f"{k}: {v}" for k, v in failures.items()))


class CheckFailed(AssertionError):
    def __init__(self, msg, rows=(), layers=()):
        self.rows, self.layers = sorted(set(int(r) for r in rows)), sorted(set(int(x) for x in layers))
        super().__init__(msg)


# ---------------------------------------------------------------- the case tables
def row_tables(lens, pos):
    """(row0 (B,), seq of every row (R,), absolute position of every row (R,))"""
    lens, pos = np.asarray(lens, np.int64), np.asarray(pos, np.int64)
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seq = np.repeat(np.arange(len(lens)), lens)
    rpos = np.concatenate([pos[b] + np.arange(lens[b]) for b in range(len(lens))]) if lens.sum() else np.zeros(0, int)
    return row0, seq, rpos


_S4 = {8: 12, 16: 24, 32: 16, 64: 56}  # a mid-page start by page size


def ragged_case(R, P):
    """(lens, pos) of R rows in 6 sequences on pages of P, a pool filled to F:
    0 rows at F-3; 1 row at P-1; 5 rows from position 0; 3 rows from F; a
    sequence from mid-page through two page boundaries to the first slot of
    the third page; the rest across key 64"""
    s4 = _S4[P]
    len4 = (s4 // P + 2) * P - s4 + 1
    len5 = R - 9 - len4
    assert len5 >= 2, (R, P)
    pos5 = 64 - min(len5 // 2, 34)
    return (np.array([0, 1, 5, 3, len4, len5], np.int32), np.array([F - 3, P - 1, 0, F, s4, pos5], np.int32))


def prefill_case(T, P):
    """gpt2_decode_prefill: 3 sequences of T rows each, from 0, 3P-1 and F"""
    return np.full(3, T, np.int32), np.array([0, 3 * P - 1, F], np.int32)


VERIFY_DRAFTS = (-1, 0, 1, 3, 7, 7, 2)


def verify_case(P):
    """gpt2_decode_verify: n_draft + 1 rows per sequence"""
    lens = np.array(VERIFY_DRAFTS, np.int32) + 1
    return lens, np.array([F - 3, P - 1, 0, F, 60, P + P // 2 + 1 if P > 8 else 13, 30], np.int32)


def case_conditions(lens, pos, P, blocks, kind="ragged"):
    """the input conditions of a case, from its tables alone (AssertionError
    otherwise).  kind "ragged" (prefill_ragged, score, score_top): all of them;
    "prefill": B x T has no sequence of 0 or 1 rows and 3 sequences of 30 rows
    share no 16-row block three ways; "verify": at most 8 rows per sequence, so
    a sequence crosses one page boundary from mid-page, not two."""
    lens, pos = np.asarray(lens, np.int64), np.asarray(pos, np.int64)
    R = int(lens.sum())
    row0, seq, _ = row_tables(lens, pos)
    live = lens > 0
    assert np.all(pos + lens <= MAX_CTX), "a sequence overflows MAX_CTX"
    assert (R + 15) // 16 == blocks, ((R + 15) // 16, blocks)
    assert np.any(live & (pos == 0)), "no sequence starts at 0"
    assert np.any(live & (pos % P == P - 1)), "no sequence starts at the last slot of a page"
    assert np.any(live & (pos == F)), "no sequence starts at F"
    assert np.any(live & (pos < 64) & (pos + lens > 64)), "no sequence crosses key 64"
    last = pos + lens - 1
    crossed = last // P - pos // P
    need = 1 if kind == "verify" else 2
    assert np.any(live & (pos % P != 0) & (crossed >= need)), f"no sequence crosses {need} page boundaries from mid-page"
    if kind != "prefill":
        assert np.any(lens == 0) and np.any(lens == 1), "no sequence of 0 rows / of 1 row"
        assert np.any(live & (pos == P - 1)), "no sequence starts at P - 1"
        assert any(len(set(seq[r:r + 16])) >= 3 for r in range(0, R, 16)), "no 16-row block holds 3 sequences"
    if R > 64:
        assert np.any(live & (row0 < 64) & (row0 + lens > 64)), "no sequence's rows straddle row 64"


# ---------------------------------------------------------------- float64 tail: LNf and the logits
def logits64(ref, xL, w_bf16=None):
    """(float64 logits (R, V), the fused GEMM's bound (R, V)) of the rows xL"""
    w_bf16 = ref.w_bf16 if w_bf16 is None else w_bf16
    a = ln(np.asarray(xL, np.float64), ref._t(14), ref._t(15))
    return gb.product_and_bound(a, ref.wte, w_bf16)


# ---------------------------------------------------------------- the checks
def check_embedding(ref, tok, lens, pos, xs):
    _, seq, rpos = row_tables(lens, pos)
    want = ref.embed(np.asarray(tok), rpos)
    same = (np.ascontiguousarray(xs[0], np.float32).view(np.uint32) == want.view(np.uint32)).all(-1)
    if not same.all():
        bad = np.flatnonzero(~same)
        raise CheckFailed(f"row {bad[0]} (sequence {seq[bad[0]]}, position {rpos[bad[0]]}) is not wte[tok] + wpe[pos] "
                          f"({len(bad)} rows in all)", rows=bad)
    return 0.0


def kv_refs(ref, lens, pos, xs):
    """ref[l][b] = (K, V) float64 (lens[b], C) from the traced layer inputs"""
    row0, _, _ = row_tables(lens, pos)
    out = []
    for l in range(ref.L):
        k, v = ref.kv_rows_exact(xs[l], l)
        out.append([(k[row0[b]:row0[b] + lens[b]], v[row0[b]:row0[b] + lens[b]]) for b in range(len(lens))])
    return out


def check_kv_layers(ref, lens, pos, xs, before, after, rtol, kv_values=True):
    refs = kv_refs(ref, lens, pos, xs) if kv_values else None
    worst = ref64.check_kv(before, after, pos, lens, ref=refs, rtol=rtol, kv_bf16=ref.kv_bf16)
    for l in range(ref.L):  # a sequence the pass did not touch: every row it has, bit for bit
        for b in np.flatnonzero(np.asarray(lens) == 0):
            for wi in range(2):
                n = min(len(before[l][b][wi]), len(after[l][b][wi]))
                assert np.array_equal(before[l][b][wi][:n].view(np.uint32), after[l][b][wi][:n].view(np.uint32)), (l, b)
    return worst


def layer_ratios(ref, lens, pos, xs, after):
    """(L, R): |layer_out - xs[l + 1]| per row over max|xs[l + 1]|"""
    row0, _, _ = row_tables(lens, pos)
    out = np.zeros((ref.L, xs.shape[1]))
    for l in range(ref.L):
        got = xs[l + 1].astype(np.float64)
        scale = np.abs(got).max()
        for b in range(len(lens)):
            n = int(lens[b])
            if n == 0:
                continue
            rows = slice(row0[b], row0[b] + n)
            K, V = after[l][b]
            want = ref.layer_out(xs[l][rows], l, [K] * n, [V] * n, pos[b] + np.arange(n) + 1)
            out[l, rows] = np.abs(want - got[rows]).max(-1) / scale
    return out


def check_layers(ref, lens, pos, xs, after, rtol):
    assert np.isfinite(xs).all(), "the traced residual stream is not finite"
    r = layer_ratios(ref, lens, pos, xs, after)
    if r.max() > rtol:
        l, row = np.unravel_index(np.argmax(r), r.shape)
        bad_l, bad_r = np.nonzero(r > rtol)
        _, seq, rpos = row_tables(lens, pos)
        raise CheckFailed(f"layer {l} row {row} (sequence {seq[row]}, position {rpos[row]}): {r.max():.2e} > {rtol:.2e} "
                          f"({len(bad_r)} (layer, row) pairs in all)", rows=bad_r, layers=bad_l)
    return float(r.max())


def check_decode(ref, lens, pos, xs, logits, next_ids, last_rows=None, x64=None):
    """logits (B, V) the engine's rows, next_ids (B,); last_rows[b]: the packed
    row gathered for sequence b (default row0 + len - 1; verify: row0 + accepted)"""
    row0, _, _ = row_tables(lens, pos)
    live = np.flatnonzero(np.asarray(lens) > 0)
    last = row0 + np.asarray(lens) - 1 if last_rows is None else np.asarray(last_rows)
    want, bound = x64 if x64 is not None else logits64(ref, xs[ref.L])
    worst, bad = 0.0, []
    for b in live:
        d = np.abs(logits[b].astype(np.float64) - want[last[b]]) / bound[last[b]]
        worst = max(worst, float(d.max()))
        if d.max() > 1.0 or int(next_ids[b]) != int(np.argmax(logits[b])):
            bad.append(b)
    if bad:
        b = bad[0]
        raise CheckFailed(f"sequence {b} (row {last[b]}): logits at {worst:.2f} of the bound, next id {int(next_ids[b])}, "
                          f"first argmax of its logits {int(np.argmax(logits[b]))}", rows=bad)
    return worst


def check_score(ref, xs, targets, logprobs, top_ids=None, alt_ids=None, alt_lps=None, x64=None):
    """targets / logprobs / top_ids (R,), alternatives (R, k): as the pass returned
    them, packed.  Returns the worst (error / bar) over the rows."""
    want, bound = x64 if x64 is not None else logits64(ref, xs[ref.L])
    R = want.shape[0]
    eps = bound.max(-1)
    targets = np.asarray(targets)
    bar = 2 * eps + sr.kernel_bound(want, targets)
    err = np.abs(np.asarray(logprobs, np.float64) - sr.logprob64(want, targets))
    ratio = err / bar
    bad = set(np.flatnonzero(ratio > 1.0).tolist())
    srt = np.sort(want, -1)
    if top_ids is not None:
        clear = srt[:, -1] - srt[:, -2] > 2 * eps
        bad |= set(np.flatnonzero(clear & (np.asarray(top_ids) != want.argmax(-1))).tolist())
    worst = float(ratio.max())
    if alt_ids is not None:
        k = alt_ids.shape[1]
        rid1, _ = tr.topk64(want, k + 1)  # one rank more: the lower neighbour of rank k - 1
        vals = np.take_along_axis(want, rid1, -1)
        rid = rid1[:, :k]
        gap_dn = vals[:, :k] - vals[:, 1:]
        gap_up = np.concatenate([np.full((R, 1), np.inf), gap_dn[:, :-1]], 1)
        clear = (gap_dn > 2 * eps[:, None]) & (gap_up > 2 * eps[:, None])
        bad |= set(np.nonzero(clear & (alt_ids != rid))[0].tolist())
        lp_at = np.take_along_axis(want, alt_ids.astype(np.int64), -1) - sr.lse64(want)[:, None]
        abar = 2 * eps[:, None] + tr.bound(want, alt_ids)
        aratio = np.abs(alt_lps.astype(np.float64) - lp_at) / abar
        bad |= set(np.nonzero(aratio > 1.0)[0].tolist())
        bad |= set(np.nonzero(np.diff(alt_lps, axis=-1) > 0)[0].tolist())
        worst = max(worst, float(aratio.max()))
    if bad:
        r = min(bad)
        raise CheckFailed(f"row {r}: log-probability error {err[r]:.2e} against a bar of {bar[r]:.2e} "
                          f"({len(bad)} rows in all, worst at {worst:.2f} of its bar)", rows=bad)
    return worst


def check_pass(ref, tok, lens, pos, xs, before, after, kv_rtol, out_rtol, logits=None, next_ids=None, last_rows=None,
               score=None, kv_values=True, collect=False):
    """every check of the module docstring.  score: dict(targets, logprobs,
    top_ids / alt_ids / alt_lps) or None.  Returns {check: worst ratio}."""
    ratios, failures = {}, {}
    x64 = logits64(ref, xs[ref.L]) if logits is not None or score is not None else None

    def run(name, fn):
        try:
            ratios[name] = fn()
        except AssertionError as e:
            failures[name] = e

    run("embedding", lambda: check_embedding(ref, tok, lens, pos, xs))
    run("kv", lambda: check_kv_layers(ref, lens, pos, xs, before, after, kv_rtol, kv_values))
    run("layer", lambda: check_layers(ref, lens, pos, xs, after, out_rtol))
    if logits is not None:
        run("decode", lambda: check_decode(ref, lens, pos, xs, logits, next_ids, last_rows, x64))
    if score is not None:
        run("score", lambda: check_score(ref, xs, x64=x64, **score))
    if collect:
        return ratios, failures
    if failures:
        raise DenseMismatch(failures)
    return ratios
