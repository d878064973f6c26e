"""The dense passes under gpt2_decode_set_prefill_attention(3): the small model
of tests/test_gpu_prefill_packed_engine.py (C = 128, NH = 2, L = 2, V = 512, page
16, peaked fp32 weights) on an fp32 pool runs prefill_ragged of (70, 5, 33, 0)
rows over a pool filled to F = 96 and a score, each traced and held to the
float64 dense model (dense_ref64.check_pass, the bars of
tests/test_gpu_dense_pass.py).  Layer 0's K/V (attention does not feed it) equals
a request-0 engine's bit for bit; on a bf16 pool request 3 is request 1 bit for
bit.
"""
import numpy as np
import pytest

import attn_ref64 as ar
import dense_ref64 as dr
import ref64
from test_gpu_kv_append import KV_RTOL, OUT_RTOL
from test_gpu_prefill_packed_engine import CFG, LENS, POS, F, P, _same_bits

pytestmark = pytest.mark.gpu


def _pass(hip, params, kv, request, entry):
    """one traced pass of `entry` on a fresh engine; returns what dense_ref64.check_pass takes"""
    m = hip.Model(CFG, params=params)
    m.decode_init(4, P, dr.MAX_CTX, kv_dtype=kv)
    want = {0: 0, 1: int(kv != hip.HPA_F32), 3: 2 if kv == hip.HPA_F32 else 1}[request]
    assert hip.prefill_plan(kv, P, 64, request) == want
    m.set_prefill_attention(request)
    R = int(LENS.sum())
    rng = np.random.default_rng(R)
    tok = rng.integers(0, CFG["V"], R).astype(np.int32)
    row0 = dr.row_tables(LENS, POS)[0]
    m.fill_random(F, seed=3)
    n_before = np.full(4, F)
    read = lambda n: [[m.read_kv(l, b, int(n[b])) for b in range(4)] for l in range(CFG["L"])]
    before = read(n_before)
    m.set_positions(POS)
    xs = m.trace_next_pass(R)
    seqs = np.split(tok, np.cumsum(LENS)[:-1])
    targets = rng.integers(0, CFG["V"], R).astype(np.int32)
    targets[(row0 + LENS - 1)[LENS > 0]] = -1
    score = None
    if entry == "prefill_ragged":
        nxt = m.prefill_ragged(seqs)
    else:
        lp, top, nxt = m.score(seqs, np.split(targets, np.cumsum(LENS)[:-1]))
        score = dict(targets=targets, logprobs=np.concatenate(lp), top_ids=np.concatenate(top))
    m.status()
    logits = m.logits()
    n_after = np.maximum(POS + LENS, n_before)
    m.set_positions(n_after)
    after = read(n_after)
    m.close()
    return dict(tok=tok, lens=LENS, pos=POS, xs=xs, before=before, after=after, logits=logits, next_ids=nxt,
                last_rows=None, score=score)


@pytest.fixture(scope="module")
def params():
    return ar.peaked_params(CFG, seed=902)


@pytest.mark.parametrize("entry", ["prefill_ragged", "score"])
def test_dense_pass_on_the_split_kernel(hip, params, entry):
    got = _pass(hip, params, hip.HPA_F32, 3, entry)
    ref = ref64.Ref64(CFG, params, w_bf16=False, kv_bf16=False)
    ratios = dr.check_pass(ref, kv_rtol=KV_RTOL[False], out_rtol=OUT_RTOL[False], **got)
    print(f"DENSEREF split {entry} kv=f32 " + " ".join(f"{k}={v:.3e}" for k, v in ratios.items()))
    base = _pass(hip, params, hip.HPA_F32, 0, entry)
    for b in range(4):
        for wi in range(2):
            assert _same_bits(got["after"][0][b][wi], base["after"][0][b][wi]), (b, "KV"[wi])


def test_bf16_pool_takes_the_packed_kernel(hip, params):
    a, b = (_pass(hip, params, hip.HPA_BF16, r, "prefill_ragged") for r in (1, 3))
    assert _same_bits(a["logits"], b["logits"]) and np.array_equal(a["next_ids"], b["next_ids"])
    assert _same_bits(a["xs"], b["xs"])
    for l in range(CFG["L"]):
        for s in range(4):
            for wi in range(2):
                assert a["after"][l][s][wi].tobytes() == b["after"][l][s][wi].tobytes(), (l, s, "KV"[wi])
