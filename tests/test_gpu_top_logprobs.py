"""Engine-level top log-probabilities: gpt2_decode_set_top_logprobs (the k
best ids of every pick's raw row, inside the captured step) and
gpt2_decode_score_top (every prompt row's k best ids through the dense route
in chunks), on the SMALL synthetic model of tests/test_gpu_score.py.

Bars:
* against the engine's own fp32 logits: ids exactly tests/top_ref64.py's, the
  log-probabilities within score_ref64's kernel bound (4e-6 + 2^-22 * magnitude);
* against the oracle's token-by-token rows: a sup-norm logit error of eps
  moves a logit and the log-sum-exp by at most eps each, so a log-probability
  at a returned id is within 2 * LOGIT_TOL of logprob64 of the oracle's row
  (LOGIT_TOL = 2e-4; bf16 weights 2e-2); the id at rank j must equal the
  oracle's where rank j is clear: the oracle's j-th value more than TIE_MARGIN
  (1e-3; bf16 4e-2) from both neighbours in sorted order.
  fp32: the seed (6) is chosen so that the oracle alone has at least half of
  all (row, rank) pairs clear (273 of 285: tests/test_top_ref64.py asserts it on
  the CPU, and the GPU test asserts it again on its own rows).
  bf16: at TIE_MARGIN 4e-2 no seed can reach one half on this model -- the top
  of 1000 logits of standard deviation 0.23 is spaced about 0.02 apart; seeds
  5..11 give 44..61 clear pairs of 285 -- so that case asserts that clear
  pairs exist in every scored sequence, like test_gpu_score.py's bf16 case.
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import score_ref64 as sr
import synth
import top_ref64 as tr

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
TIE_MARGIN = 1e-3
SMALL = dict(maxT=256, V=1000, L=2, NH=2, C=128)
V = SMALL["V"]


@pytest.fixture(scope="module")
def params():
    return synth.params(SMALL, seed=11)


def _model(hip, params, B, P=16, **kw):
    m = hip.Model(SMALL, params=params)
    m.decode_init(B, P, SMALL["maxT"], **kw)
    return m


def _seqs(rng, lens):
    return [rng.integers(0, V, n).astype(np.int32) for n in lens]


def _oracle_rows(params, seq, pre_tok=(), page_seed=1, bf16=False):
    """the oracle's logits at every token of one sequence, decoded token by
    token after the tokens pre_tok: (len(seq), V)"""
    c = oc.cfg(SMALL["maxT"], V, SMALL["L"], SMALL["NH"], SMALL["C"])
    orc = oc.PagedDecoder(params, c, 1, 16, SMALL["maxT"], page_seed=page_seed, kv_bf16=bf16, w_bf16=bf16)
    for t in pre_tok:
        orc.step(np.array([t], np.int32))
    rows = np.zeros((len(seq), V), np.float32)
    for t in range(len(seq)):
        rows[t] = orc.step(seq[t:t + 1])[1][0]
    orc.close()
    return rows


def _check_top(m, k, rows=None):
    """top_logprobs() against topk64(logits()): ids exact, lps within the kernel bound"""
    x = m.logits()
    ids, lps = m.top_logprobs()
    assert ids.shape == (m.B, k) and lps.shape == (m.B, k)
    rows = np.arange(m.B) if rows is None else np.asarray(rows)
    rid, rlp = tr.topk64(x, k)
    assert np.array_equal(ids[rows], rid[rows]), (ids[rows], rid[rows])
    err = np.abs(lps.astype(np.float64) - rlp)
    assert np.all(err[rows] <= tr.bound(x, rid)[rows]), err
    assert np.all(np.diff(lps[rows], axis=-1) <= 0)
    return ids, lps


def test_off_by_default_and_bad_k(hip, params):
    m = _model(hip, params, 2)
    tok = m.step(np.array([1, 2], np.int32))
    with pytest.raises(RuntimeError):
        m.top_logprobs()
    for bad in (21, -1):
        with pytest.raises(RuntimeError):
            m.set_top_logprobs(bad)
        assert hip.lib().gpt2_decode_top_logprobs_k(m.h) == 0
        with pytest.raises(RuntimeError):
            m.top_logprobs()
    m.set_top_logprobs(3)
    with pytest.raises(RuntimeError):
        m.set_top_logprobs(21)
    assert hip.lib().gpt2_decode_top_logprobs_k(m.h) == 3  # a refused k changes nothing
    m.step(tok)
    _check_top(m, 3)
    m.close()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("mode", ["greedy", "filtered"])
@pytest.mark.parametrize("k", [5, 20])
def test_decode_top_logprobs(hip, params, graph, mode, k):
    """after every step top_logprobs() is the exact top k of logits() (the raw
    distribution in every sampling mode)"""
    B = 4
    m = _model(hip, params, B)
    m.set_graph(graph)
    if mode == "filtered":
        m.set_sampling(True, seed=3, filtered=True)
        m.set_sampling_params(-1, temperature=0.8, top_k=40, top_p=0.9)
        m.set_sampling_params(1, temperature=0.0)
    greedy_rows = np.arange(B) if mode == "greedy" else np.array([1])
    m.set_top_logprobs(k)
    m.set_logprobs(True)
    tok = np.random.default_rng(10).integers(0, V, B).astype(np.int32)
    for _ in range(6):
        tok = m.step(tok)
        ids, lps = _check_top(m, k)
        assert np.array_equal(ids[greedy_rows, 0], tok[greedy_rows])
        # the chosen id's own log-probability (hpa_logprob_rows) where it is among the alternatives: each
        # kernel within one bound of the float64 value
        lp1 = m.logprobs()
        x = m.logits()
        for b in range(B):
            hit = np.flatnonzero(ids[b] == tok[b])
            if len(hit):
                assert abs(float(lps[b, hit[0]]) - float(lp1[b])) <= 2 * sr.kernel_bound(x, tok)[b]
    # ragged prefill with one sequence left out: its values stay
    before = m.top_logprobs()
    seqs = _seqs(np.random.default_rng(12), [9, 0, 1, 17])
    m.prefill_ragged(seqs)
    after = _check_top(m, k, rows=[0, 2, 3])
    assert np.array_equal(after[0][1], before[0][1])
    assert np.array_equal(after[1][1].view(np.int32), before[1][1].view(np.int32))
    # a score pick updates the others too
    m.score(seqs)
    after2 = _check_top(m, k, rows=[0, 2, 3])
    assert np.array_equal(after2[0][1], before[0][1])
    # k: 5 <-> 20, then off, then on again
    k2 = 25 - k
    m.set_top_logprobs(k2)
    tok = m.step(None)
    _check_top(m, k2)
    m.set_top_logprobs(0)
    tok = m.step(tok)
    with pytest.raises(RuntimeError):
        m.top_logprobs()
    m.set_top_logprobs(k)
    tok = m.step(tok)
    _check_top(m, k)
    m.close()


def test_processors_do_not_change_the_alternatives(hip, params):
    """a hard ban on one sequence's raw argmax: the pick avoids it, entry 0 is
    still the raw argmax (the alternatives are the raw model distribution)"""
    B = 3
    tok = np.array([11, 12, 13], np.int32)
    probe = _model(hip, params, B)
    probe.step(tok)
    raw_best = sr.first_argmax(probe.logits())
    probe.close()
    m = _model(hip, params, B)
    m.set_processors(True)
    m.set_logit_bias(1, [int(raw_best[1])], [-np.inf])
    m.set_top_logprobs(5)
    nxt = m.step(tok)
    ids, _ = _check_top(m, 5)
    assert np.array_equal(sr.first_argmax(m.logits()), raw_best)
    assert ids[1, 0] == raw_best[1] and nxt[1] != raw_best[1]
    assert nxt[0] == ids[0, 0] and nxt[2] == ids[2, 0]
    m.close()


@pytest.mark.parametrize("graph", [False, True])
def test_off_is_the_engine_without_it(hip, params, graph):
    """toggled on and off again, the next 4 steps' ids and logits equal a model
    that never enabled it, bit for bit"""
    B = 3
    a, b = _model(hip, params, B), _model(hip, params, B)
    tok = np.array([5, 6, 7], np.int32)
    for m in (a, b):
        m.set_graph(graph)
    ta, tb = a.step(tok), b.step(tok)
    a.set_top_logprobs(20)
    ta, tb = a.step(ta), b.step(tb)
    _check_top(a, 20)
    a.set_top_logprobs(0)
    for _ in range(4):
        ta, tb = a.step(ta), b.step(tb)
        assert np.array_equal(ta, tb)
        assert np.array_equal(a.logits().view(np.int32), b.logits().view(np.int32))
    a.close()
    b.close()


def test_after_verify_the_pending_tokens_row(hip, params):
    B = 3
    m = _model(hip, params, B)
    m.set_top_logprobs(5)
    tok = m.step(np.array([21, 22, 23], np.int32))
    before = m.top_logprobs()
    acc, toks, _ = m.verify([[int(tok[0])], None, [1, 2, 3]])
    ids, _ = _check_top(m, 5, rows=[0, 2])
    for b in (0, 2):
        assert ids[b, 0] == toks[b][-1]  # the model's own next token: the new pending id
    assert np.array_equal(ids[1], before[0][1])
    m.close()


def _clear_ranks(rows, k, tie):
    """(rows, k) bool: the j-th sorted value is more than tie from both neighbours"""
    s = -np.sort(-rows.astype(np.float64), -1)[:, :k + 1]
    below = (s[:, :-1] - s[:, 1:]) > tie
    above = np.concatenate([np.ones((len(rows), 1), bool), below[:, :-1]], 1)
    return below & above


def _score_top_case(hip, params, tol, tie, bf16, need_half):
    lens, pre, k = [37, 0, 20], 5, 5
    B = len(lens)
    kw = dict(kv_dtype=hip.HPA_BF16, w_dtype=hip.HPA_BF16) if bf16 else {}
    rng = np.random.default_rng(6)
    pre_tok = rng.integers(0, V, (pre, B)).astype(np.int32)
    seqs = _seqs(rng, lens)
    targets = [rng.integers(0, V, n).astype(np.int32) for n in lens]
    for t in targets:
        t[::7] = -1
    m, twin, rag = (_model(hip, params, B, **kw) for _ in range(3))
    for t in range(pre):
        for e in (m, twin, rag):
            e.step(pre_tok[t])
    lp, ids, lps, nxt = m.score_top(seqs, k, targets)
    lp_ref, _, nxt_ref = twin.score(seqs, targets)
    assert np.array_equal(m.positions(), pre + np.asarray(lens))
    # the state afterwards is prefill_ragged's
    nxt_rag = rag.prefill_ragged(seqs)
    assert np.array_equal(nxt, nxt_rag) and np.array_equal(nxt, nxt_ref)
    assert np.array_equal(m.positions(), rag.positions())
    assert np.array_equal(m.logits().view(np.int32), rag.logits().view(np.int32))
    for l in range(SMALL["L"]):
        for s in range(B):
            ka, va = m.read_kv(l, s, pre + lens[s])
            kb, vb = rag.read_kv(l, s, pre + lens[s])
            assert np.array_equal(ka.view(np.int32), kb.view(np.int32))
            assert np.array_equal(va.view(np.int32), vb.view(np.int32))
    worst = worst_t = 0.0
    n_clear = n_all = 0
    for b in range(B):
        if not lens[b]:
            assert len(lp[b]) == 0 and ids[b].shape == (0, k) and lps[b].shape == (0, k)
            continue
        rows = _oracle_rows(params, seqs[b], pre_tok[:, b], page_seed=b + 1, bf16=bf16)
        ref = rows.astype(np.float64) - sr.lse64(rows)[:, None]
        err = np.abs(lps[b] - np.take_along_axis(ref, ids[b].astype(np.int64), -1))
        worst = max(worst, float(err.max()))
        assert np.all(np.diff(lps[b], axis=-1) <= 0)
        assert all(len(set(r.tolist())) == k for r in ids[b])
        worst_t = max(worst_t, float(np.abs(lp[b] - lp_ref[b]).max()))
        assert np.all(lp[b][targets[b] < 0] == 0.0)
        clear = _clear_ranks(rows, k, tie)
        assert clear.any()
        n_clear += int(clear.sum())
        n_all += clear.size
        assert np.array_equal(ids[b][clear], tr.topk64(rows, k)[0][clear])
    print(f"score_top vs oracle: worst |lp diff| {worst:.3e} (bar {2 * tol:.1e}), vs score {worst_t:.3e} "
          f"(bar {4 * tol:.1e}), clear ranks {n_clear} of {n_all}")
    assert worst <= 2 * tol
    assert worst_t <= 4 * tol
    if need_half:
        assert 2 * n_clear >= n_all
    for e in (m, twin, rag):
        e.close()


def test_score_top_matches_oracle(hip, params):
    """ragged lens with an untouched sequence, starts at position 5 (mid-page)"""
    _score_top_case(hip, params, LOGIT_TOL, TIE_MARGIN, bf16=False, need_half=True)


def test_score_top_matches_oracle_bf16_weights(hip, params):
    _score_top_case(hip, params, 2e-2, 4e-2, bf16=True, need_half=False)


def test_score_top_chunk_seam(hip, params):
    """57 rows in chunks of 16 (4 chunks, the last of 9 rows) against the
    default single chunk: equal ids, the log-probabilities within twice the
    kernel bound (each side within one of the same logits' float64 value); the
    same setting twice: identical bits"""
    lens, k = [30, 27], 5
    seqs = _seqs(np.random.default_rng(7), lens)
    outs = []
    for chunk in (0, 16, 16):
        m = _model(hip, params, 2)
        m.set_score_chunk(chunk)
        lp, ids, lps, nxt = m.score_top(seqs, k)
        outs.append((np.concatenate(lp), np.concatenate(ids), np.concatenate(lps), nxt, m.logits()))
        m.close()
    ref = outs[0]
    # the bound's magnitude from the oracle's logits of the same rows (within LOGIT_TOL of the engine's)
    rows = np.concatenate([_oracle_rows(params, s) for s in seqs])
    mag = np.maximum(np.abs(sr.lse64(rows))[:, None], np.abs(np.take_along_axis(rows, ref[1].astype(np.int64), -1)))
    bound = 4e-6 + 2.0 ** -22 * (mag + LOGIT_TOL)
    for o in outs[1:]:
        assert np.array_equal(o[1], ref[1]) and np.array_equal(o[3], ref[3])
        assert np.all(np.abs(o[2].astype(np.float64) - ref[2]) <= 2 * bound)
        assert np.all(np.abs(o[0].astype(np.float64) - ref[0]) <= 2 * bound.max(-1))
        assert np.array_equal(o[4].view(np.int32), ref[4].view(np.int32))
    for i in (0, 2):
        assert np.array_equal(outs[1][i].view(np.int32), outs[2][i].view(np.int32))


def test_score_top_rejections_change_nothing(hip, params):
    m = _model(hip, params, 2)
    m.step(np.array([1, 2], np.int32))
    seqs = _seqs(np.random.default_rng(9), [20, 40])
    pos, free = m.positions().copy(), m.free_pages()
    for k in (0, 21):
        with pytest.raises(RuntimeError):
            m.score_top(seqs, k)
        assert np.array_equal(m.positions(), pos) and m.free_pages() == free
    tg = [np.zeros(20, np.int32), np.zeros(40, np.int32)]
    tg[1][39] = V
    with pytest.raises(RuntimeError):
        m.score_top(seqs, 5, tg)
    assert np.array_equal(m.positions(), pos) and m.free_pages() == free
    lp, ids, lps, _ = m.score_top(seqs, 5)  # still usable
    assert ids[1].shape == (40, 5) and np.array_equal(m.positions(), pos + [20, 40])
    m.close()
