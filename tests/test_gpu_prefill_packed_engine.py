"""The dense passes under gpt2_decode_set_prefill_attention(1): a small model
(C = 128, NH = 2, L = 2, V = 512, page 16, peaked fp32 weights) on a bf16 and an
fp8 pool runs prefill_ragged of (70, 5, 33, 0) rows over a pool filled to F = 96,
a score and a chain verify of 4 rows, each traced and held to the float64 dense
model (dense_ref64.check_pass, the bars of tests/test_gpu_dense_pass.py).  Layer
0's K/V (attention does not feed it) equals a request-0 engine's bit for bit; on
an fp32 pool request 1 changes no bit.
"""
import numpy as np
import pytest

import attn_ref64 as ar
import dense_ref64 as dr
import ref64
from test_gpu_kv_append import KV_RTOL, OUT_RTOL
from test_gpu_kv_fp8 import OUT_RTOL as FP8_OUT_RTOL

pytestmark = pytest.mark.gpu

CFG = dict(maxT=dr.MAX_CTX, V=512, L=2, NH=2, C=128)
P, F = 16, dr.F
LENS = np.array([70, 5, 33, 0], np.int32)
POS = np.array([0, P - 1, 40, F - 3], np.int32)
VLENS = np.array([4, 4, 4, 0], np.int32)  # verify: the pending id and 3 drafts
VPOS = np.array([0, P - 1, 62, F - 3], np.int32)


def _pass(hip, params, kv, request, entry):
    """one traced pass of `entry` on a fresh engine; returns what dense_ref64.check_pass takes"""
    m = hip.Model(CFG, params=params)
    m.decode_init(4, P, dr.MAX_CTX, kv_dtype=kv)
    if kv == hip.HPA_FP8:
        m.set_kv_scales(np.array([[0.37, 2.0], [1.0, 0.125]], np.float32), np.array([[2.0, 0.37], [0.125, 1.0]], np.float32))
    assert hip.prefill_plan(kv, P, 64, request) == int(request == 1 and kv != hip.HPA_F32)
    m.set_prefill_attention(request)
    lens, pos = (VLENS, VPOS) if entry == "verify" else (LENS, POS)
    R = int(lens.sum())
    rng = np.random.default_rng(R)
    tok = rng.integers(0, CFG["V"], R).astype(np.int32)
    row0 = dr.row_tables(lens, pos)[0]
    m.fill_random(F, seed=3)
    n_before = np.full(4, F)
    if entry == "verify":
        m.set_verify_attention(1)  # the prefill-kernel route on every pool
        tok[row0[:3]] = m.step(rng.integers(0, CFG["V"], 4).astype(np.int32))[:3]  # pending ids; writes row F
        n_before = np.full(4, F + 1)
    read = lambda n: [[m.read_kv(l, b, int(n[b])) for b in range(4)] for l in range(CFG["L"])]
    before = read(n_before)
    m.set_positions(pos)
    xs = m.trace_next_pass(R)
    seqs = np.split(tok, np.cumsum(lens)[:-1])
    targets = rng.integers(0, CFG["V"], R).astype(np.int32)
    targets[(row0 + lens - 1)[lens > 0]] = -1
    score = last_rows = None
    if entry == "prefill_ragged":
        nxt = m.prefill_ragged(seqs)
    elif entry == "score":
        lp, top, nxt = m.score(seqs, np.split(targets, np.cumsum(lens)[:-1]))
        score = dict(targets=targets, logprobs=np.concatenate(lp), top_ids=np.concatenate(top))
    else:
        acc, toks, lps = m.verify([s[1:].tolist() if len(s) else None for s in seqs], want_logprobs=True)
        last_rows = row0 + np.array([-1 if a is None else a for a in acc])
        nxt = np.array([0 if t is None else t[-1] for t in toks])
        for b in range(3):
            targets[row0[b]:row0[b] + 3] = seqs[b][1:]
        score = dict(targets=targets, logprobs=np.concatenate([np.append(x, 0.0) for x in lps[:3]]).astype(np.float32))
    m.status()
    logits = m.logits()
    n_after = np.maximum(pos + lens, n_before)
    m.set_positions(n_after)
    after = read(n_after)
    m.close()
    return dict(tok=tok, lens=lens, pos=pos, xs=xs, before=before, after=after, logits=logits, next_ids=nxt,
                last_rows=last_rows, score=score)


@pytest.fixture(scope="module")
def params():
    return ar.peaked_params(CFG, seed=902)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("entry", ["prefill_ragged", "score", "verify"])
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_dense_pass_on_the_packed_kernel(hip, params, kv, entry):
    dt = {"bf16": hip.HPA_BF16, "fp8": hip.HPA_FP8}[kv]
    got = _pass(hip, params, dt, 1, entry)
    ref = ref64.Ref64(CFG, params, w_bf16=False, kv_bf16=kv == "bf16")
    ratios = dr.check_pass(ref, kv_rtol=KV_RTOL[False], out_rtol=FP8_OUT_RTOL if kv == "fp8" else OUT_RTOL[False],
                           kv_values=kv != "fp8", **got)
    print(f"DENSEREF packed {entry} kv={kv} " + " ".join(f"{k}={v:.3e}" for k, v in ratios.items()))
    base = _pass(hip, params, dt, 0, entry)
    for b in range(4):
        for wi in range(2):
            assert _same_bits(got["after"][0][b][wi], base["after"][0][b][wi]), (b, "KV"[wi])


def test_fp32_pool_is_untouched_by_the_request(hip, params):
    a, b = (_pass(hip, params, hip.HPA_F32, r, "prefill_ragged") for r in (0, 1))
    assert _same_bits(a["logits"], b["logits"]) and np.array_equal(a["next_ids"], b["next_ids"])
    assert _same_bits(a["xs"], b["xs"])
    for l in range(CFG["L"]):
        for s in range(4):
            for wi in range(2):
                assert _same_bits(a["after"][l][s][wi], b["after"][l][s][wi]), (l, s, "KV"[wi])
