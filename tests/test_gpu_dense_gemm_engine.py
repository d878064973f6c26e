"""The dense passes under gpt2_decode_set_dense_gemm(1): the small model of
tests/test_gpu_prefill_packed_engine.py (C = 128, NH = 2, L = 2, V = 512, page 16,
peaked fp32 weights; K = 128 and 512) runs prefill_ragged of (70, 5, 33, 0) rows
over a pool filled to F = 96 and a score with every layer and head GEMM on the
split-operand kernel (hpa_gemm_fused variant 7), each traced and held to the
float64 dense model under the bars tests/test_gpu_dense_pass.py applies to fp32
weights; once on a bf16 pool (the QKV append).  A verify pass accepts and emits
what plain greedy decoding emits, and request 0 afterwards gives back a fresh
engine's bits.
"""
import numpy as np
import pytest

import attn_ref64 as ar
import dense_ref64 as dr
import ref64
from test_gpu_kv_append import KV_RTOL, OUT_RTOL
from test_gpu_prefill_packed_engine import CFG, LENS, POS, F, P, _same_bits

pytestmark = pytest.mark.gpu


def _pass(hip, params, kv, requests, entry):
    """a fresh engine, then per request the same traced pass of `entry` from the same
    state; returns what dense_ref64.check_pass takes, of the last request"""
    m = hip.Model(CFG, params=params)
    m.decode_init(4, P, dr.MAX_CTX, kv_dtype=kv)
    R = int(LENS.sum())
    rng = np.random.default_rng(R)
    tok = rng.integers(0, CFG["V"], R).astype(np.int32)
    row0 = dr.row_tables(LENS, POS)[0]
    seqs = np.split(tok, np.cumsum(LENS)[:-1])
    targets = rng.integers(0, CFG["V"], R).astype(np.int32)
    targets[(row0 + LENS - 1)[LENS > 0]] = -1
    read = lambda n: [[m.read_kv(l, b, int(n[b])) for b in range(4)] for l in range(CFG["L"])]
    for request in requests:
        assert hip.dense_gemm_plan(hip.HPA_F32, CFG["C"], request) == request
        m.set_dense_gemm(request)
        m.fill_random(F, seed=3)
        before = read(np.full(4, F))
        m.set_positions(POS)
        xs, score = m.trace_next_pass(R), None
        if entry == "prefill_ragged":
            nxt = m.prefill_ragged(seqs)
        else:
            lp, top, nxt = m.score(seqs, np.split(targets, np.cumsum(LENS)[:-1]))
            score = dict(targets=targets, logprobs=np.concatenate(lp), top_ids=np.concatenate(top))
        m.status()
        logits = m.logits()
        n_after = np.maximum(POS + LENS, F)
        m.set_positions(n_after)
        after = read(n_after)
    m.close()
    return dict(tok=tok, lens=LENS, pos=POS, xs=xs, before=before, after=after, logits=logits, next_ids=nxt,
                last_rows=None, score=score)


@pytest.fixture(scope="module")
def params():
    return ar.peaked_params(CFG, seed=902)


@pytest.mark.parametrize("kv,entry", [("f32", "prefill_ragged"), ("f32", "score"), ("bf16", "prefill_ragged")])
def test_dense_pass_on_the_split_gemm(hip, params, kv, entry):
    got = _pass(hip, params, {"f32": hip.HPA_F32, "bf16": hip.HPA_BF16}[kv], [1], entry)
    ref = ref64.Ref64(CFG, params, w_bf16=False, kv_bf16=kv == "bf16")
    ratios = dr.check_pass(ref, kv_rtol=KV_RTOL[False], out_rtol=OUT_RTOL[False], **got)
    print(f"DENSEREF split-gemm {entry} kv={kv} " + " ".join(f"{k}={v:.3e}" for k, v in ratios.items()))


def test_request_0_restores_a_fresh_engines_bits(hip, params):
    a, b = (_pass(hip, params, hip.HPA_F32, r, "prefill_ragged") for r in ([1, 0], [0]))
    assert _same_bits(a["logits"], b["logits"]) and np.array_equal(a["next_ids"], b["next_ids"])
    assert _same_bits(a["xs"], b["xs"])
    for l in range(CFG["L"]):
        for s in range(4):
            for wi in range(2):
                assert _same_bits(a["after"][l][s][wi], b["after"][l][s][wi]), (l, s, "KV"[wi])


def test_verify_emits_the_greedy_ids(hip, params):
    tok = np.random.default_rng(5).integers(0, CFG["V"], (4, 21)).astype(np.int32)
    runs = []
    for request in (0, 1):
        m = hip.Model(CFG, params=params)
        m.decode_init(4, P, dr.MAX_CTX)
        m.set_dense_gemm(request)
        first = m.prefill(tok)
        if request == 0:
            runs.append(np.stack([first] + [m.step(None) for _ in range(4)]))  # (5, B): the pending id, then 4 greedy ids
        else:
            acc, toks, _ = m.verify([runs[0][1:4, b].tolist() for b in range(4)])
            assert np.array_equal(first, runs[0][0]) and acc == [3] * 4
            assert all(toks[b] == runs[0][1:5, b].tolist() for b in range(4))
        m.close()
