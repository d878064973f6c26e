"""The engine's greedy stream where every logit is negative, as with real
GPT-2 weights: pick_inputs.negative_logit_params (synth.params with wte
shifted along u = (+1, -1, ...) and lnfb against it, so every logit moves by
about -delta beta C and no embedding row's mean moves).

All cases: L = 2, page 16, a short ragged prefill (1..9 tokens), then 6 greedy
steps on random fed tokens, eager and under set_graph(True).  The oracle is
handed the K/V the engine's prefill stored, so both decode at the same ragged
positions on identical caches.

  * every id (the prefill's too) is < V and is the first argmax of
    m.logits(), bit for bit, on every step
  * graph ids and logits are bit-identical to the eager ones
  * ids equal the oracle's outside near-ties (test_gpu_decode.IdCheck's rule)
  * on one traced step the logits are within gemm_bounds.product_and_bound of
    the float64 LNf(xs[L]) . wte^T of the engine's own final residual (the
    decode suite's LOGIT_TOL was set for logits near 0 and is not used here)
  * condition, on the oracle's logits of every compared row: maximum <= -1,
    at least 8 distinct greedy ids
  * B = 5 only: score() against the oracle, one verify() of oracle drafts
    accepts them all, entry 0 of set_top_logprobs(5) is the picked id

Cases (hpa_logits_kernel names the logits path: 4 resident, 1 looped, 6
stream-K): C = 768, V = 5009 at B = 5 / 64 (resident forms 16 / 12), B = 70
(looped), B = 40 with bf16 weights (the bf16 chain and bf16 logits); C = 1600,
NH = 25, V = 2001 at B = 33 (stream-K).

Measured (MI355X; oracle logit range, distinct greedy ids, traced step's worst
|gpu - f64| / bound; the file runs in 2.7 s):
  B = 5 [-16.1, -6.6] 16 0.035 | B = 64 [-15.7, -6.6] 27 0.065 | B = 70 [-16.1, -6.7] 26 0.067
  B = 40 bf16 [-16.2, -6.9] 25 0.022 | C = 1600 B = 33 [-20.8, -10.8] 27 0.024
  no id >= V, no near-tie row in fp32, 29 of 240 with bf16 weights; score() 9.9e-6 against a bar of 8.1e-4
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import pick_inputs as pi
import score_ref64 as sr
import synth
from gemm_bounds import product_and_bound
from test_gpu_decode import BF16_EXEMPT, IdCheck

pytestmark = pytest.mark.gpu

C768 = dict(maxT=64, V=5009, L=2, NH=12, C=768)
C1600 = dict(maxT=64, V=2001, L=2, NH=25, C=1600)
P, STEPS, TRACED = 16, 6, 2
# the decode suite's bar on |engine - oracle| logits: still what the layers ahead of LNf contribute (the
# fixture leaves them alone); the final GEMM's share is added from its own bound in the B = 5 test
LAYERS_TOL = 2e-4


@pytest.fixture(scope="module")
def params768():
    return pi.negative_logit_params(C768, 7, 0.01, 1.5)


@pytest.fixture(scope="module")
def params1600():
    return pi.negative_logit_params(C1600, 7, 0.01, 1.0)


def _tensor(cfgd, params, i):
    off, sz = synth.offsets(cfgd), synth.sizes(cfgd)
    return params[off[i]:off[i] + sz[i]]


def _logits64(cfgd, params, xL, w_bf16):
    """(float64 LNf(xL) . wte^T, the fused GEMM's bound) of final-residual rows xL"""
    a = pi.ln64(xL, _tensor(cfgd, params, 14), _tensor(cfgd, params, 15))
    return product_and_bound(a, _tensor(cfgd, params, 0).reshape(cfgd["V"], cfgd["C"]), w_bf16)


def _own_pick(m, ids, V):
    """ids against the engine's own logits; returns them"""
    x = m.logits()
    pi.check_pick(ids, x, V)
    return x


def _seqs(cfgd, B, seed):
    rng = np.random.default_rng(seed)
    lens = 1 + (np.arange(B) * 5) % 9
    return [rng.integers(0, cfgd["V"], n).astype(np.int32) for n in lens], lens


def _model(hip, cfgd, params, B, w_bf16, graph):
    m = hip.Model(cfgd, params=params)
    m.decode_init(B, P, cfgd["maxT"], w_dtype=hip.HPA_BF16 if w_bf16 else hip.HPA_F32)
    m.set_graph(graph)
    return m


def _run(hip, cfgd, params, B, w_bf16, kernel, form, chain):
    """kernel: what hpa_logits_kernel names for the fp32 logits; form: the layer
    loop's form (0 five launches, 3 attention + chain, 4 the bf16 chain);
    chain: the planner's chain form for the shape (6, 8; 0 none)"""
    V = cfgd["V"]
    assert w_bf16 or hip.lib().hpa_logits_kernel(B, V, cfgd["C"]) == kernel
    assert hip.layer_plan(1, B, cfgd["C"], cfgd["NH"], cfgd["maxT"], w_bf16=w_bf16)["chain"] == chain
    seqs, lens = _seqs(cfgd, B, seed=B)
    feed = np.random.default_rng(B + 1).integers(0, V, (STEPS, B)).astype(np.int32)
    eager, graph = (_model(hip, cfgd, params, B, w_bf16, g) for g in (False, True))
    assert eager.layer_form() == form and graph.layer_form() == form, (eager.layer_form(), form)
    n_e, n_g = eager.prefill_ragged(seqs), graph.prefill_ragged(seqs)
    x = _own_pick(eager, n_e, V)
    assert np.array_equal(n_e, n_g) and np.array_equal(x.view(np.uint32), graph.logits().view(np.uint32))
    assert x.max() <= -1.0
    orc = oc.PagedDecoder(params, oc.cfg(cfgd["maxT"], V, cfgd["L"], cfgd["NH"], cfgd["C"]), B, P, cfgd["maxT"],
                          page_seed=B, w_bf16=w_bf16)
    for l in range(cfgd["L"]):
        for b in range(B):
            k, v = eager.read_kv(l, b, int(lens[b]))
            orc.set_kv(l, b, k, v)
    chk, rows, ratio = IdCheck(), [], None
    for s in range(STEPS):
        o_next, o_logits = orc.step(feed[s])
        if s == TRACED:  # the eager step with the residual stream handed back
            g_next, xs = eager.step_traced(feed[s])
        else:
            g_next = eager.step(feed[s])
        x = _own_pick(eager, g_next, V)
        if s == TRACED:
            ref, bound = _logits64(cfgd, params, xs[cfgd["L"]], w_bf16)
            ratio = float((np.abs(x - ref) / bound).max())
            assert ratio <= 1.0, ratio
        gn = graph.step(feed[s])
        assert np.array_equal(gn, g_next), s
        assert np.array_equal(graph.logits().view(np.uint32), x.view(np.uint32)), s
        chk.add(x, o_logits, g_next, o_next)
        rows.append(o_logits.copy())
    assert np.array_equal(eager.positions(), lens + STEPS)
    chk.verify(np.inf, BF16_EXEMPT if w_bf16 else 0.02)
    for m in (eager, graph, orc):
        m.close()
    return rows, ratio


def _report(name, rows, ratio):
    lo, hi, distinct = pi.check_negative_regime(np.concatenate([r.reshape(-1, r.shape[-1]) for r in rows]))
    print(f"{name}: oracle logits in [{lo:.1f}, {hi:.1f}], {distinct} distinct greedy ids; "
          f"traced step worst |gpu - f64| / bound {ratio:.3f}")


@pytest.mark.parametrize("B,kernel,form,chain", [(64, 4, 3, 6), (70, 1, 0, 0)])
def test_negative_logits_c768(hip, params768, B, kernel, form, chain):
    """B = 64: the resident ring form and chain form 6; B = 70: the looped logits, five launches per layer"""
    rows, ratio = _run(hip, C768, params768, B, False, kernel, form, chain)
    _report(f"C=768 V=5009 B={B}", rows, ratio)


def test_negative_logits_c768_bf16_weights(hip, params768):
    rows, ratio = _run(hip, C768, params768, 40, True, None, 4, 0)
    _report("C=768 V=5009 B=40 bf16 weights", rows, ratio)


def test_negative_logits_c1600_stream_k(hip, params1600):
    rows, ratio = _run(hip, C1600, params1600, 33, False, 6, 3, 8)
    _report("C=1600 V=2001 B=33", rows, ratio)


def test_negative_logits_c768_b5_with_score_verify_top(hip, params768):
    """B = 5 (the 16-wave resident form), and on the same weights: score()
    against single-sequence oracles decoded token by token (top ids exact
    outside near-ties; log-probabilities within 2 eps of the float64
    log-softmax of the oracle's logits, eps the bar on the logits themselves:
    a sup-norm logit error of eps moves the target's logit and the
    log-sum-exp by at most eps each); one verify() of three oracle-drafted
    ids per sequence accepts them all; entry 0 of top_logprobs() is the pick.

    eps = LAYERS_TOL + 2 * the final GEMM's worst bound on the scored rows
    (gemm_bounds, from the engine's own traced residual): the engine's logits
    are within that bound of the float64 product of its residual, the
    oracle's fp32 dot products within it of theirs, and the two residuals
    differ by what the layers ahead contribute, LAYERS_TOL as in the decode
    suite."""
    cfgd, params, B = C768, params768, 5
    V = cfgd["V"]
    rows, ratio = _run(hip, cfgd, params, B, False, 4, 3, 6)
    m = _model(hip, cfgd, params, B, False, False)
    rng = np.random.default_rng(3)
    lens = [9, 16, 1, 12, 7]
    seqs = [rng.integers(0, V, n).astype(np.int32) for n in lens]
    targets = [rng.integers(0, V, n).astype(np.int32) for n in lens]
    for t in targets:
        t[::5] = -1
    targets[1][3], targets[3][0] = V - 1, 0
    xs = m.trace_next_pass(sum(lens))
    lp, top, nxt = m.score(seqs, targets)
    _own_pick(m, nxt, V)
    bound = _logits64(cfgd, params, xs[cfgd["L"]], False)[1]
    eps = LAYERS_TOL + 2 * float(bound.max())
    orcs, worst = [], 0.0
    for b in range(B):
        o = oc.PagedDecoder(params, oc.cfg(cfgd["maxT"], V, cfgd["L"], cfgd["NH"], cfgd["C"]), 1, P, cfgd["maxT"],
                            page_seed=b + 1)
        orows = np.stack([o.step(seqs[b][t:t + 1])[1][0].copy() for t in range(lens[b])])
        rows.append(orows)
        worst = max(worst, float(np.abs(lp[b] - sr.logprob64(orows, targets[b])).max()))
        assert np.all(lp[b][targets[b] < 0] == 0.0)
        clear = pi.top2_margin(orows) > 2 * eps
        assert np.array_equal(top[b][clear], sr.first_argmax(orows)[clear]) and np.all(top[b] < V)
        assert not clear[-1] or nxt[b] == top[b][-1]
        orcs.append(o)
    print(f"score vs oracle: worst |logprob diff| {worst:.3e} (bar {2 * eps:.3e})")
    assert worst <= 2 * eps
    # drafts: the oracle's next three greedy ids after the engine's pending id
    drafts, sure = [], []
    for b in range(B):
        tok, d, ok = np.array([nxt[b]], np.int32), [], True
        for _ in range(3):
            tok, ol = orcs[b].step(tok)
            rows.append(ol.copy())
            ok = ok and pi.top2_margin(ol)[0] > 2 * eps
            d.append(int(tok[0]))
        drafts.append(d)
        sure.append(ok)
        orcs[b].close()
    acc, toks, _ = m.verify(drafts)
    assert sum(sure) >= B - 1, sure  # at most one sequence drafted through a near-tie
    for b in range(B):
        assert all(0 <= t < V for t in toks[b])
        if sure[b]:
            assert acc[b] == 3 and toks[b][:3] == drafts[b], (b, acc[b], toks[b], drafts[b])
    m.set_top_logprobs(5)
    for _ in range(2):
        ids = m.step(None)
        x = _own_pick(m, ids, V)
        tids, tlps = m.top_logprobs()
        assert np.array_equal(tids[:, 0], ids) and np.all((tids >= 0) & (tids < V))
        assert np.all(np.abs(tlps[:, 0] - sr.logprob64(x, ids)) <= sr.kernel_bound(x, ids))
    m.close()
    _report("C=768 V=5009 B=5 (+ score / verify rows)", rows, ratio)
