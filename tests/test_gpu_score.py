"""Engine-level scoring: gpt2_decode_score (every prompt token's
log-probability and greedy id through the fused SCORE GEMM) and
gpt2_decode_set_logprobs (the log-probability of each id a pick chose).

Bars:
* against the oracle's token-by-token decode: a sup-norm logit error of eps
  moves the target's logit and the log-sum-exp by at most eps each, so the
  log-probabilities are within 2 * LOGIT_TOL (LOGIT_TOL = 2e-4, the bar of
  test_gpu_prefill.py) of the float64 log-softmax of the oracle's logits;
  greedy ids exact where the oracle's top-2 margin exceeds TIE_MARGIN;
* against the engine's own fp32 logits: the kernel bound of
  tests/score_ref64.py (4e-6 + 2^-22 * magnitude).
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import score_ref64 as sr
import synth

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


def _oracle_case(hip, params, lens, pre, tol, tie, bf16=False):
    B, P = len(lens), 16
    kw = dict(kv_dtype=hip.HPA_BF16, w_dtype=hip.HPA_BF16) if bf16 else {}
    m = _model(hip, params, B, P, **kw)
    rng = np.random.default_rng(5)
    pre_tok = rng.integers(0, V, (pre, B)).astype(np.int32)
    for t in range(pre):
        m.step(pre_tok[t])
    seqs = _seqs(rng, lens)
    targets = [rng.integers(0, V, n).astype(np.int32) for n in lens]
    for t in targets:
        t[::7] = -1
    lp, top, nxt = m.score(seqs, targets)
    assert np.array_equal(m.positions(), pre + np.asarray(lens))
    worst = 0.0
    for b in range(B):  # one single-sequence oracle per sequence, token by token
        rows = _oracle_rows(params, seqs[b], pre_tok[:, b], page_seed=b + 1, bf16=bf16)
        if not lens[b]:
            assert len(lp[b]) == 0 and len(top[b]) == 0
            continue
        err = np.abs(lp[b] - sr.logprob64(rows, targets[b]))
        worst = max(worst, float(err.max()))
        assert np.all(lp[b][targets[b] < 0] == 0.0)
        s = np.sort(rows, -1)
        clear = s[:, -1] - s[:, -2] > tie
        assert clear.any()
        assert np.array_equal(top[b][clear], sr.first_argmax(rows)[clear])
        assert not clear[-1] or nxt[b] == top[b][-1]  # the last row's greedy id is the pick
    print(f"score vs oracle: worst |logprob diff| {worst:.3e} (bar {2 * tol:.1e})")
    assert worst <= 2 * tol
    m.close()


def test_score_matches_oracle(hip, params):
    """ragged lens with an untouched sequence, starts at position 5 (mid-page)"""
    _oracle_case(hip, params, [37, 0, 20], pre=5, tol=LOGIT_TOL, tie=TIE_MARGIN)


def test_score_matches_oracle_bf16_weights(hip, params):
    _oracle_case(hip, params, [37, 0, 20], pre=5, tol=2e-2, tie=4e-2, bf16=True)


def test_score_leaves_the_state_prefill_ragged_leaves(hip, params):
    """score == prefill_ragged for everything a prefill changes: positions,
    next ids, logits and K/V bit for bit, and the next 4 decode steps"""
    lens = [37, 0, 20]
    rng = np.random.default_rng(6)
    pre_tok = rng.integers(0, V, (3, 3)).astype(np.int32)
    seqs = _seqs(rng, lens)
    a, b = _model(hip, params, 3), _model(hip, params, 3)
    for t in range(3):
        assert np.array_equal(a.step(pre_tok[t]), b.step(pre_tok[t]))
    na = a.score(seqs)[2]
    nb = b.prefill_ragged(seqs)
    assert np.array_equal(na, nb)
    assert np.array_equal(a.positions(), b.positions())
    assert np.array_equal(a.logits().view(np.int32), b.logits().view(np.int32))
    for l in range(SMALL["L"]):
        for s in range(3):
            ka, va = a.read_kv(l, s, 3 + lens[s])
            kb, vb = b.read_kv(l, s, 3 + lens[s])
            assert np.array_equal(ka.view(np.int32), kb.view(np.int32))
            assert np.array_equal(va.view(np.int32), vb.view(np.int32))
    for _ in range(4):
        assert np.array_equal(a.step(None), b.step(None))
        assert np.array_equal(a.logits().view(np.int32), b.logits().view(np.int32))
    a.close()
    b.close()


def test_score_chunk_seam(hip, params):
    """57 rows in chunks of 16 (4 chunks, the last of 9 rows) against the
    default single chunk: the log-probabilities within twice the kernel bound
    (each side within one of the same logits' float64 value), equal greedy
    ids; the same setting twice: identical bits"""
    lens = [30, 27]
    seqs = _seqs(np.random.default_rng(7), lens)
    outs = []
    for chunk in (0, 16, 16, 32):
        m = _model(hip, params, 2)
        m.set_score_chunk(chunk)
        lp, top, nxt = m.score(seqs)
        outs.append((np.concatenate(lp), np.concatenate(top), nxt, m.logits()))
        m.close()
    ref = outs[0]
    # the bound's magnitude from the oracle's logits of the same rows (within LOGIT_TOL of the engine's)
    rows = np.concatenate([_oracle_rows(params, s) for s in seqs])
    tgt = np.concatenate([np.concatenate([s[1:], [-1]]) for s in seqs])
    bound = 4e-6 + 2.0 ** -22 * (np.maximum(np.abs(sr.lse64(rows)), np.abs(rows[np.arange(57), tgt])) + LOGIT_TOL)
    for o in outs[1:]:
        assert np.all(np.abs(o[0] - ref[0]) <= 2 * bound)
        assert np.array_equal(o[1], ref[1]) and np.array_equal(o[2], ref[2])
        assert np.array_equal(o[3].view(np.int32), ref[3].view(np.int32))
    assert np.array_equal(outs[1][0].view(np.int32), outs[2][0].view(np.int32))


def test_score_shifted_targets_and_own_logits(hip, params):
    """targets=None is the shift (token t+1 scores position t, the last has
    none), and the last row's values agree with the engine's own logits"""
    lens = [19, 33]
    seqs = _seqs(np.random.default_rng(8), lens)
    a, b = _model(hip, params, 2), _model(hip, params, 2)
    lp_a, top_a, n_a = a.score(seqs)
    explicit = [np.concatenate([s[1:], [-1]]).astype(np.int32) for s in seqs]
    lp_b, top_b, n_b = b.score(seqs, explicit)
    for s in range(2):
        assert np.array_equal(lp_a[s].view(np.int32), lp_b[s].view(np.int32))
        assert np.array_equal(top_a[s], top_b[s])
        assert lp_a[s][-1] == 0.0 and np.all(lp_a[s][:-1] < 0)
    assert np.array_equal(n_a, n_b)
    # the last row again with a real target: within the kernel bound of log-softmax(model.logits())
    x = a.logits()
    last_t = np.array([3, V - 1], np.int32)
    c = _model(hip, params, 2)
    tg = [np.full(n, -1, np.int32) for n in lens]
    for s in range(2):
        tg[s][-1] = last_t[s]
    lp_c, top_c, _ = c.score(seqs, tg)
    got = np.array([lp_c[0][-1], lp_c[1][-1]])
    # (the decode logits GEMM may sum a row's K in another order than the SCORE GEMM: each is within
    # LOGIT_TOL of the oracle, so the two log-probabilities are within 4 * LOGIT_TOL plus the kernel bound)
    assert np.all(np.abs(got - sr.logprob64(x, last_t)) <= sr.kernel_bound(x, last_t) + 4 * LOGIT_TOL)
    srt = np.sort(x, -1)
    clear = srt[:, -1] - srt[:, -2] > TIE_MARGIN
    assert np.array_equal(np.array([top_c[0][-1], top_c[1][-1]])[clear], sr.first_argmax(x)[clear])
    for m in (a, b, c):
        m.close()


def test_score_rejections_change_nothing(hip, params):
    m = _model(hip, params, 2)
    m.step(np.array([1, 2], np.int32))
    seqs = _seqs(np.random.default_rng(9), [20, 40])
    pos, free = m.positions().copy(), m.free_pages()
    for bad in (V, -2):
        tg = [np.zeros(20, np.int32), np.zeros(40, np.int32)]
        tg[1][39] = bad
        with pytest.raises(RuntimeError):
            m.score(seqs, tg)
        assert np.array_equal(m.positions(), pos) and m.free_pages() == free
    for rows in (24, -16):
        with pytest.raises(RuntimeError):
            m.set_score_chunk(rows)
    assert np.array_equal(m.positions(), pos) and m.free_pages() == free
    lp, _, _ = m.score(seqs)  # still usable, default chunk still in force
    assert len(lp[1]) == 40 and np.array_equal(m.positions(), pos + [20, 40])
    m.close()


def _check_lp(m, ids, rows=None):
    x = m.logits()
    lp = m.logprobs()
    rows = np.arange(len(ids)) if rows is None else rows
    err = np.abs(lp.astype(np.float64) - sr.logprob64(x, ids))
    assert np.all(err[rows] <= sr.kernel_bound(x, ids)[rows]), err
    return lp


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("mode", ["greedy", "filtered"])
def test_decode_logprobs(hip, params, graph, mode):
    """after every step logprobs() is the float64 log-softmax of logits() at
    the returned ids (raw distribution in every sampling mode), within the
    kernel bound"""
    B = 4
    m = _model(hip, params, B)
    m.set_graph(graph)
    if mode == "filtered":
        m.set_sampling(True, seed=3, filtered=True)
        m.set_sampling_params(-1, temperature=0.8, top_k=40, top_p=0.9)
        m.set_sampling_params(1, temperature=0.0)
    with pytest.raises(RuntimeError):
        m.logprobs()  # off by default
    m.set_logprobs(True)
    tok = np.random.default_rng(10).integers(0, V, B).astype(np.int32)
    for _ in range(6):
        tok = m.step(tok)
        lp = _check_lp(m, tok)
        assert np.all(lp <= 0)
    # ragged prefill with one sequence left out: its value stays
    before = m.logprobs()
    seqs = _seqs(np.random.default_rng(12), [9, 0, 1, 17])
    nxt = m.prefill_ragged(seqs)
    after = _check_lp(m, nxt, rows=np.array([0, 2, 3]))
    assert after[1] == before[1]
    # score picks too
    nxt = m.score(seqs)[2]
    _check_lp(m, nxt, rows=np.array([0, 2, 3]))
    # off, on again, a step
    m.set_logprobs(False)
    tok = m.step(None)
    with pytest.raises(RuntimeError):
        m.logprobs()
    m.set_logprobs(True)
    tok = m.step(tok)
    _check_lp(m, tok)
    m.close()


@pytest.mark.parametrize("graph", [False, True])
def test_logprobs_off_is_the_engine_without_it(hip, params, graph):
    """toggled on and off again, the next 4 steps' ids and logits equal a model
    that never enabled it, bit for bit"""
    B = 3
    a, b = _model(hip, params, B), _model(hip, params, B)
    tok = np.array([5, 6, 7], np.int32)
    for m in (a, b):
        m.set_graph(graph)
    ta, tb = a.step(tok), b.step(tok)
    a.set_logprobs(True)
    ta, tb = a.step(ta), b.step(tb)
    a.set_logprobs(False)
    for _ in range(4):
        ta, tb = a.step(ta), b.step(tb)
        assert np.array_equal(ta, tb)
        assert np.array_equal(a.logits().view(np.int32), b.logits().view(np.int32))
    a.close()
    b.close()
