"""The dense ragged pass (dec_prefill_rows / dec_prefill_layers: prefill,
prefill_ragged, score, score_top, verify) pinned to float64 layer by layer, on
the pass's own inputs, through the trace of gpt2_decode_trace_next_pass.

Every case opens a 3-layer model of a real width (V = 1000, max_ctx = 160),
asserts layer_form() and the kernel choice it is named for
(hpa_fused_pick_bf16_ares, gpt2_decode_verify_plan), fills the pool to F = 96,
snapshots every layer's rows, lowers the positions to the case's ragged starts
(dense_ref64.ragged_case / prefill_case / verify_case; their input conditions
are asserted on the CPU by tests/test_dense_ref64.py and again here), runs one
traced pass and hands the trace, the pool's rows before and after, the logits
rows, the next ids and the scores to dense_ref64.check_pass: embedding exact,
K/V rows of every layer (stray / unwritten / value), every layer's output on
the pool's own K/V with the causal mask as the context length, the gathered
decode rows against float64 LNf . wte^T, and every row's log-probability.

Weights: attn_ref64.peaked_params with fp32 weights (a wrong key is an O(1)
error; attn_ref64.input_conditions asserted on layer 0: median largest softmax
weight >= 0.25 over the rows with at least 8 keys, E <= 40), synth.params with
bf16 weights, as tests/test_gpu_kv_append.py does for that mode.

Bars, all the project's own: K/V rows KV_RTOL[w_bf16] and layer outputs
OUT_RTOL[w_bf16] of tests/test_gpu_kv_append.py (already capped by
FP32_LAYER_RTOL / BF16_LAYER_RTOL); the fp8 pool holds its layer outputs to
tests/test_gpu_kv_fp8.py's OUT_RTOL and has no K/V value check, as in
tests/test_gpu_layer_hard.py; logits within the fused GEMM's bound
(tests/gemm_bounds.py); log-probabilities within 2 eps_r + the scoring
kernels' bound.  The fp32 emulation of tests/test_dense_ref64.py, which the
checker accepts as correct, sits at 4.5e-07 (K/V) and 7.9e-07 (outputs) on these
tables, so no bar had to be derived from it.

Deviations from a uniform table: the B x T entry has no sequence of 0 or 1 rows
and the verify entry has at most 8 rows per sequence (one page boundary from
mid-page, not two); dense_ref64.case_conditions says which conditions each
kind holds.  A verify pass needs pending ids: they come from one decode step
after fill_random, and the drafts are the engine's own greedy continuation
from the case's positions (7 further steps, then the state is rebuilt), with
one draft of two sequences replaced so that acceptance stops inside the row
block.

Each case prints one DENSEREF line.  Measured on the MI355X (K/V and output
ratios raw; logits and score as a fraction of their bar):

  entry           C     R    P   w / pool     K/V rows   outputs    logits  score
  prefill_ragged  768   70   16  f32 / f32    4.16e-07   8.79e-07   0.010   -
  prefill_ragged  768   90   64  f32 / f32    3.93e-07   1.12e-06   0.008   -
  prefill_ragged  768   120  8   f32 / bf16   1.92e-07   8.69e-07   0.009   -
  prefill_ragged  768   70   16  f32 / fp8    -          8.01e-07   0.009   -
  prefill_ragged  768   70   8   bf16 / bf16  3.43e-08   9.59e-04   0.004   -
  prefill_ragged  768   130  8   bf16 / bf16  1.53e-04   1.38e-03   0.003   -
  prefill_ragged  1024  70   32  f32 / f32    4.18e-07   8.77e-07   0.005   -
  prefill (3x30)  768   90   16  f32 / f32    4.12e-07   7.88e-07   0.009   -
  score           768   90   16  f32 / f32    3.77e-07   7.92e-07   0.009   0.004
  score           768   90   16  bf16 / bf16  6.65e-05   4.87e-04   0.005   0.002
  score_top k=5   768   90   16  f32 / f32    3.77e-07   7.92e-07   0.009   0.008
  score_top k=5   768   90   16  bf16 / bf16  6.65e-05   4.87e-04   0.005   0.004
  verify auto     768   26   16  f32 / f32    3.63e-07   8.27e-07   0.012   0.005
  verify req. 1   768   26   16  f32 / f32    3.63e-07   9.21e-07   0.008   0.007
  verify auto     768   26   8   f32 / bf16   1.44e-07   7.23e-07   0.009   0.004

(bf16 pools: K/V after the store's half ulp is taken off; set_score_chunk(32)
and the default chunk give the same figures.  Bars: K/V 4.68e-06 / 6.44e-04 and
outputs 4.96e-06 / 4.00e-03 for fp32 / bf16 weights, fp8 outputs 2.61e-06.)
"""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
import dense_ref64 as dr
import ref64
import synth
from test_gpu_kv_append import KV_RTOL, OUT_RTOL
from test_gpu_kv_fp8 import OUT_RTOL as FP8_OUT_RTOL
from test_gpu_kv_fp8 import _engine_scales

pytestmark = pytest.mark.gpu

F, MAX_CTX = dr.F, dr.MAX_CTX
L, V = 3, 1000

_params = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_params():
    yield
    _params.clear()


def _model_params(C, NH, w_bf16):
    cfgd = dict(maxT=MAX_CTX, V=V, L=L, NH=NH, C=C)
    key = (C, w_bf16)
    if key not in _params:
        _params.clear()  # one model at a time
        _params[key] = synth.params(cfgd, seed=700 + NH) if w_bf16 else ar.peaked_params(cfgd, seed=900 + NH)
    return cfgd, _params[key]


def _open(hip, C, NH, B, P, w, kv):
    """fp32 weights: chain form 6 at C = 768, chain form 8 at C = 1024 (form 3);
    bf16 weights: the bf16 chain (form 4).  The dense pass is the same under each."""
    w_bf16 = w == "bf16"
    cfgd, params = _model_params(C, NH, w_bf16)
    m = hip.Model(cfgd, params=params)
    m.decode_init(B, P, MAX_CTX, kv_dtype={"f32": hip.HPA_F32, "bf16": hip.HPA_BF16, "fp8": hip.HPA_FP8}[kv],
                  w_dtype=hip.HPA_BF16 if w_bf16 else hip.HPA_F32)
    if not w_bf16:
        m.set_layer_kernel(5 if C == 768 else 6)
    assert m.layer_form() == (4 if w_bf16 else 3), m.layer_form()
    if kv == "fp8":
        m.set_kv_scales(*_engine_scales(NH))  # every sequence at position 0
    return cfgd, params, m


def _read_all(m, n):
    return [[m.read_kv(l, b, int(n[b])) for b in range(m.B)] for l in range(L)]


def _assert_gemm_choice(hip, R, w_bf16):
    """bf16 weights: which of qkv / attproj / fc / fcproj take the A-resident kernel at R rows"""
    if not w_bf16:
        return
    pk = (ctypes.c_int * 3)()
    pick = [hip.lib().hpa_fused_pick_bf16_ares(R, n, k, pk) for n, k in ((2304, 768), (768, 768), (3072, 768), (768, 3072))]
    assert pick == ([1, 0, 1, 0] if (R + 15) // 16 >= 8 else [0, 0, 0, 0]), (R, pick)


def _split(flat, lens):
    return np.split(np.asarray(flat), np.cumsum(lens)[:-1])


def _run_case(hip, entry, C, NH, table, P, w, kv, blocks, kind="ragged", chunk=0, k=5, vreq=0, verify_kernel=None):
    lens, pos = table
    dr.case_conditions(lens, pos, P, blocks, kind)
    B, R = len(lens), int(lens.sum())
    w_bf16 = w == "bf16"
    cfgd, params, m = _open(hip, C, NH, B, P, w, kv)
    _assert_gemm_choice(hip, R, w_bf16)
    ref = ref64.Ref64(cfgd, params, w_bf16=w_bf16, kv_bf16=kv == "bf16")
    rng = np.random.default_rng(1000 * C + 10 * R + P)
    row0 = dr.row_tables(lens, pos)[0]
    tok = rng.integers(0, V, R).astype(np.int32)
    targets = rng.integers(0, V, R).astype(np.int32)
    targets[(row0 + lens - 1)[lens > 0]] = -1  # a sequence's last row: no target
    m.fill_random(F, seed=C + R)
    n_before = np.full(B, F)
    drafts = None
    if entry == "verify":
        assert hip.verify_plan(int(lens.max()), m_kv_dtype(hip, kv), P, 64, vreq) == verify_kernel
        m.set_verify_attention(vreq)
        tok0 = rng.integers(0, V, B).astype(np.int32)
        pend = m.step(tok0)  # pending ids; writes row F of every sequence
        m.set_positions(pos)
        greedy = np.stack([m.step(None) for _ in range(7)])  # (7, B): the continuation from (pos, pending)
        m.fill_random(F, seed=C + R)
        assert np.array_equal(m.step(tok0), pend)
        n_before = np.full(B, F + 1)
        drafts = [None if n == 0 else greedy[:n - 1, b].copy() for b, n in enumerate(lens)]
        drafts[5][3] = (drafts[5][3] + 1) % V  # acceptance stops at 3 of 7
        drafts[6][0] = (drafts[6][0] + 1) % V  # and at 0 of 2
        for b in np.flatnonzero(lens > 0):
            tok[row0[b]] = pend[b]
            tok[row0[b] + 1:row0[b] + lens[b]] = drafts[b]
            targets[row0[b]:row0[b] + lens[b] - 1] = drafts[b]
    before = _read_all(m, n_before)
    m.set_positions(pos)
    xs = m.trace_next_pass(R)
    seqs = _split(tok, lens)
    score = last_rows = None
    if entry == "prefill_ragged":
        nxt = m.prefill_ragged(seqs)
    elif entry == "prefill":
        nxt = m.prefill(tok.reshape(B, -1))
    elif entry == "score":
        m.set_score_chunk(chunk)
        lp, top, nxt = m.score(seqs, _split(targets, lens))
        score = dict(targets=targets, logprobs=np.concatenate(lp), top_ids=np.concatenate(top))
    elif entry == "score_top":
        m.set_score_chunk(chunk)
        lp, ids, lps, nxt = m.score_top(seqs, k, _split(targets, lens))
        score = dict(targets=targets, logprobs=np.concatenate(lp), alt_ids=np.concatenate(ids), alt_lps=np.concatenate(lps))
    else:
        acc, toks, lps = m.verify([None if d is None else d.tolist() for d in drafts], want_logprobs=True)
        accv = np.array([-1 if a is None else a for a in acc])
        # the drafts are the engine's own continuation: some sequence accepts past its first row, and the
        # replaced drafts stop the two others, so "row0 + accepted" is not always a sequence's first or last row
        assert accv[5] <= 3 and accv[6] == 0 and accv[4] >= 1, accv
        print(f"DENSEREF verify accepted={accv.tolist()}")
        last_rows = row0 + accv
        nxt = np.array([0 if t is None else t[-1] for t in toks])
        for b in np.flatnonzero(lens > 0):
            assert toks[b][:-1] == drafts[b][:accv[b]].tolist(), b
        lpk = np.zeros(R, np.float32)
        for b in np.flatnonzero(lens > 0):
            lpk[row0[b]:row0[b] + lens[b] - 1] = lps[b]
        score = dict(targets=targets, logprobs=lpk)
    m.status()
    moved = lens if entry != "verify" else np.where(lens > 0, last_rows - row0 + 1, 0)
    assert np.array_equal(m.positions(), pos + moved)
    logits = m.logits()
    n_after = np.maximum(pos + lens, n_before)
    m.set_positions(n_after)  # keeps pages: only makes the rows readable again
    after = _read_all(m, n_after)
    # the hook disarmed itself: a second pass leaves the trace as it is
    snap = xs.copy()
    m.set_positions(pos)
    m.prefill_ragged(seqs)
    assert np.array_equal(xs.view(np.uint32), snap.view(np.uint32))
    m.close()

    _, seq, rpos = dr.row_tables(lens, pos)
    if not w_bf16:  # the inputs are what the module says they are (float64 over the pool's rows)
        wmax, E = ar.input_conditions(ref, xs[0], [after[0][b][0] for b in seq], [after[0][b][1] for b in seq], rpos + 1)
        assert np.median(wmax[rpos + 1 >= 8]) >= 0.25, float(np.median(wmax[rpos + 1 >= 8]))
        assert E.max() <= 40.0, float(E.max())
    out_rtol = FP8_OUT_RTOL if kv == "fp8" else OUT_RTOL[w_bf16]
    ratios, failures = dr.check_pass(ref, tok, lens, pos, xs, before, after, KV_RTOL[w_bf16], out_rtol, logits=logits,
                                     next_ids=nxt, last_rows=last_rows, score=score, kv_values=kv != "fp8", collect=True)
    print(f"DENSEREF {entry} C={C} R={R} P={P} w={w} kv={kv} chunk={chunk} vreq={vreq} "
          + " ".join(f"{name}={ratios[name]:.3e}" if name in ratios else f"{name}=FAILED"
                     for name in ("kv", "layer", "decode", "score") if name in ratios or name in failures))
    if failures:
        raise dr.DenseMismatch(failures)


def m_kv_dtype(hip, kv):
    return {"f32": hip.HPA_F32, "bf16": hip.HPA_BF16, "fp8": hip.HPA_FP8}[kv]


@pytest.mark.parametrize("C,NH,R,P,w,kv,blocks", [
    pytest.param(768, 12, 70, 16, "f32", "f32", 5, id="C768-R70-P16-f32-f32"),      # row blocks 4 -> 1, col tiles 2 -> 1
    pytest.param(768, 12, 90, 64, "f32", "f32", 6, id="C768-R90-P64-f32-f32"),      # row blocks 2
    pytest.param(768, 12, 120, 8, "f32", "bf16", 8, id="C768-R120-P8-f32-bf16"),    # row blocks 4, col tiles 2
    pytest.param(768, 12, 70, 16, "f32", "fp8", 5, id="C768-R70-P16-f32-fp8"),      # fp8 stores
    pytest.param(768, 12, 70, 8, "bf16", "bf16", 5, id="C768-R70-P8-bf16-bf16"),    # looped bf16 kernel
    pytest.param(768, 12, 130, 8, "bf16", "bf16", 9, id="C768-R130-P8-bf16-bf16"),  # A-resident qkv / fc
    pytest.param(1024, 16, 70, 32, "f32", "f32", 5, id="C1024-R70-P32-f32-f32"),    # K = 1024 / 4096
])
def test_prefill_ragged(hip, C, NH, R, P, w, kv, blocks):
    _run_case(hip, "prefill_ragged", C, NH, dr.ragged_case(R, P), P, w, kv, blocks)


def test_prefill_b_by_t(hip):
    """gpt2_decode_prefill: 3 x 30 rows from ragged starts"""
    _run_case(hip, "prefill", 768, 12, dr.prefill_case(30, 16), 16, "f32", "f32", 6, kind="prefill")


@pytest.mark.parametrize("chunk", [32, 0], ids=["chunk32", "default_chunk"])
@pytest.mark.parametrize("w", ["f32", "bf16"])
@pytest.mark.parametrize("entry", ["score", "score_top"])
def test_score(hip, entry, w, chunk):
    """90 rows: set_score_chunk(32) gathers chunks of 32, 32 and 26 rows"""
    _run_case(hip, entry, 768, 12, dr.ragged_case(90, 16), 16, w, w, 6, chunk=chunk, k=5)


@pytest.mark.parametrize("P,kv,vreq,kernel", [(16, "f32", 0, 1), (16, "f32", 1, 0), (8, "bf16", 0, 0)],
                         ids=["few_row_kernel", "request_prefill_kernel", "bf16_pool_prefill_kernel"])
def test_verify(hip, P, kv, vreq, kernel):
    _run_case(hip, "verify", 768, 12, dr.verify_case(P), P, "f32", kv, 2, kind="verify", vreq=vreq, verify_kernel=kernel)


def _traced_and_not(hip, traced, floats=None):
    lens, pos = dr.ragged_case(70, 16)
    B, R = len(lens), int(lens.sum())
    _, _, m = _open(hip, 768, 12, B, 16, "f32", "f32")
    tok = np.random.default_rng(4).integers(0, V, R).astype(np.int32)
    m.fill_random(F, seed=9)
    before = _read_all(m, np.full(B, F))
    m.set_positions(pos)
    xs = m.trace_next_pass(R, floats) if traced else None  # held by the caller while the pass runs
    return m, lens, pos, _split(tok, lens), before, xs


def test_trace_changes_no_bit(hip):
    got = []
    for traced in (False, True):
        m, lens, pos, seqs, _, xs = _traced_and_not(hip, traced)
        nxt = m.prefill_ragged(seqs)
        m.status()
        assert xs is None or (np.isfinite(xs).all() and xs[-1].any())  # the traced pass did fill its buffer
        logits = m.logits()
        n = np.maximum(pos + lens, F)
        m.set_positions(n)
        got.append((nxt, logits, _read_all(m, n)))
        m.close()
    (n0, l0, kv0), (n1, l1, kv1) = got
    assert np.array_equal(n0, n1)
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))
    for l in range(L):
        for b in range(len(kv0[l])):
            for wi in range(2):
                assert np.array_equal(kv0[l][b][wi].view(np.uint32), kv1[l][b][wi].view(np.uint32)), (l, b, "KV"[wi])


def test_undersized_trace_is_refused(hip):
    """one float short: the pass is refused with positions and pool rows
    unchanged, the hook is disarmed, and the next pass runs untraced"""
    lens, pos = dr.ragged_case(70, 16)
    need = (L + 1) * 70 * 768
    m, lens, pos, seqs, before, xs = _traced_and_not(hip, True, floats=need - 1)
    free0 = m.free_pages()
    with pytest.raises(RuntimeError):
        m.prefill_ragged(seqs)
    m.status()
    assert np.array_equal(m.positions(), pos)
    assert m.free_pages() == free0  # no page taken
    assert not xs.any()  # and nothing written
    m.set_positions(np.full(len(lens), F, np.int32))
    after = _read_all(m, np.full(len(lens), F))
    for l in range(L):
        for b in range(len(lens)):
            for wi in range(2):
                assert np.array_equal(before[l][b][wi].view(np.uint32), after[l][b][wi].view(np.uint32)), (l, b)
    m.set_positions(pos)
    m.prefill_ragged(seqs)  # disarmed: runs
    assert np.array_equal(m.positions(), pos + lens)
    m.close()
