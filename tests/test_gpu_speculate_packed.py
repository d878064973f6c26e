"""Speculation on bf16 and fp8 KV pools under verify-attention request 3
(hpa_paged_attention_verify_packed, hpa_pool_compact_path_packed): the small
model of tests/test_gpu_speculate.py with (bf16 weights + bf16 pool) and (fp32
weights + fp8 pool, per-head scales none of which is 1).

The truth is plain greedy decoding on the same engine configuration.  Ids are
compared only inside a window whose every greedy margin clears TIE, asserted
first; TOL / TIE are the bf16 bars of tests/test_gpu_speculate.py, and the two
attention routes may differ by 2 TOL as in its "SPEC routes" check."""
import numpy as np
import pytest

from test_gpu_kv_fp8 import HEAD_SCALES
from test_gpu_score import SMALL, V
from test_gpu_speculate import B, P, _forced, _pending, params  # noqa: F401

pytestmark = pytest.mark.gpu
TOL, TIE, K, STEPS = 2e-2, 4e-2, 7, 40
CONFIGS = ("bf16", "fp8")


def _open(hip, params, name, request, stream=(), s0=0):
    """an engine under `request` fed the forced tokens and stream[:s0]; returns (engine, its next ids)"""
    m = hip.Model(SMALL, params=params)
    if name == "bf16":
        m.decode_init(B, P, SMALL["maxT"], kv_dtype=hip.HPA_BF16, w_dtype=hip.HPA_BF16)
    else:
        m.decode_init(B, P, SMALL["maxT"], kv_dtype=hip.HPA_FP8)
        lh = np.arange(SMALL["L"])[:, None] + np.arange(SMALL["NH"])[None, :]
        m.set_kv_scales(np.ascontiguousarray(HEAD_SCALES[1:][lh % 2]),
                        np.ascontiguousarray(HEAD_SCALES[1:][(lh + 1) % 2]))
    m.set_verify_attention(request)
    for ids in _forced():
        nxt = m.step(ids)
    if s0:
        m.prefill_ragged([stream[:s0, b] for b in range(B)])
        nxt = _pending(hip, m)
        assert np.array_equal(nxt, stream[s0])
    return m, nxt


@pytest.fixture(scope="module")
def truths():
    return {}


def _truth(hip, params, name, truths):
    """(stream (STEPS, B), s0): plain greedy ids after the forced tokens; s0: the
    first window of K + 2 steps whose margins all clear TIE"""
    if name not in truths:
        m, nxt = _open(hip, params, name, 0)
        stream, logits = np.zeros((STEPS, B), np.int32), np.zeros((STEPS, B, V), np.float32)
        for t in range(STEPS):
            stream[t], logits[t] = nxt, m.logits()
            nxt = m.step(None)
        m.close()
        s = np.sort(logits, -1)
        margin = (s[..., -1] - s[..., -2]).min(1)
        ok = [s0 for s0 in range(1, STEPS - K - 2) if margin[s0:s0 + K + 2].min() > TIE]
        assert ok, f"no window of {K + 2} greedy steps clears the tie margin: {margin}"
        truths[name] = (stream, ok[0])
    return truths[name]


@pytest.mark.parametrize("name", CONFIGS)
def test_chain_request_3_equals_request_0(hip, params, truths, name):
    """the same state through verify(drafts) under request 0 (the prefill
    kernel) and request 3: accepted counts and ids equal, logits within 2 TOL
    (sequence 1's third draft is wrong); verify_sampled under request 3 at
    temperature 0 returns the greedy pass's results exactly.  First the plan:
    request 3 gives 1 where requests 0 and 2 give 0"""
    dt = hip.HPA_BF16 if name == "bf16" else hip.HPA_FP8
    for k in (1, 4, 8):
        assert [hip.verify_plan(k, dt, P, request=r) for r in (0, 2, 3)] == [0, 0, 1]
    assert [hip.verify_plan(8, d, 8, request=3) for d in (hip.HPA_FP8, hip.HPA_BF16, hip.HPA_F32)] == [0, 1, 1]
    assert hip.verify_plan(9, dt, P, request=3) == 0
    stream, s0 = _truth(hip, params, name, truths)
    drafts = [stream[s0 + 1:s0 + 1 + K, b].tolist() for b in range(B)]
    drafts[1][2] = (drafts[1][2] + 1) % V
    outs = []
    for request, sampled in ((0, False), (3, False), (3, True)):
        m = _open(hip, params, name, request, stream, s0)[0]
        if sampled:
            m.set_sampling(True, seed=7, filtered=True)
            m.set_sampling_params(temperature=0.0)
        acc, toks = (m.verify_sampled if sampled else m.verify)(drafts)[:2]
        outs.append((acc, toks, m.logits()))
        m.close()
    assert outs[0][0] == outs[1][0] == outs[2][0] == [K, 2, K, K]
    assert outs[0][1] == outs[1][1] == outs[2][1]
    for b in (0, 2, 3):
        assert outs[1][1][b] == stream[s0 + 1:s0 + K + 2, b].tolist()
    d = float(np.abs(outs[0][2] - outs[1][2]).max())
    print(f"SPECPACKED {name} routes: |logit diff| {d:.3e} (bar {2 * TOL:.0e})")
    assert d <= 2 * TOL


def _tree(t):
    """7 drafts around the true tokens t[0..2]: three wrong children of the root before the right one (node 4),
    then node 5 and, after a wrong sibling, node 7 -- the path's sources (slots 4, 5, 7) outlive the move to 1, 2, 3"""
    t1, t2, t3 = (int(x) for x in t)
    return [(t1 + 1) % V, (t1 + 2) % V, (t1 + 3) % V, t1, t2, (t3 + 1) % V, t3], [0, 0, 0, 0, 4, 5, 5]


@pytest.mark.parametrize("sampled", (False, True))
@pytest.mark.parametrize("name", CONFIGS)
def test_tree_request_3(hip, params, truths, name, sampled):
    """refused under request 0 with the state unchanged; under request 3 the
    pass continues from the off-first-branch sibling (nodes 4, 5, 7), emits
    plain greedy decoding's ids, and slots pos + 1 .. pos + 3 hold exactly what
    the nodes' own slots hold.  sampled: verify_tree_sampled at temperature 0, the same results"""
    stream, s0 = _truth(hip, params, name, truths)
    m = _open(hip, params, name, 0, stream, s0)[0]
    if sampled:
        m.set_sampling(True, seed=7, filtered=True)
        m.set_sampling_params(temperature=0.0)
    run = m.verify_tree_sampled if sampled else m.verify_tree
    trees = [_tree(stream[s0 + 1:s0 + 4, b]) for b in range(B)]
    pos0, pend0 = m.positions().copy(), _pending(hip, m)
    with pytest.raises(Exception):
        run(trees)
    assert np.array_equal(m.positions(), pos0) and np.array_equal(_pending(hip, m), pend0)
    m.set_verify_attention(3)
    acc, toks, nodes = run(trees)[:3]
    assert acc == [3] * B
    for b in range(B):
        assert nodes[b] == [4, 5, 7], b
        assert toks[b] == stream[s0 + 1:s0 + 5, b].tolist(), b
    assert np.array_equal(m.positions(), pos0 + 4)
    assert np.array_equal(_pending(hip, m), stream[s0 + 4])
    m.set_positions(pos0 + 8)  # keeps pages: only makes the nodes' own slots (left as the pass wrote them) readable
    for layer in range(SMALL["L"]):
        for b in range(B):
            for rows in m.read_kv(layer, b, int(pos0[b]) + 8):
                own, moved = rows[pos0[b] + [4, 5, 7]], rows[pos0[b] + [1, 2, 3]]
                assert np.isfinite(own).all() and np.array_equal(own, moved), (layer, b)
    m.set_positions(pos0 + 4)
    for t in range(3):  # decoding goes on from the compacted state
        nxt = m.step(None)
        if not sampled:
            assert np.array_equal(nxt, stream[s0 + 5 + t]), t
    m.close()
