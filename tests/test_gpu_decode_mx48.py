"""The decode engine as W4A8 (gpt2_decode_init_w, HPA_FP4A8) against the float64 model of the dequantised
weights with every layer-GEMM input through the mirror quantiser (pagedattn.quantize_mxfp8_rows), at the
geometry, cases and bars of tests/test_gpu_decode_fp4w.py (the MXFP4 codes and scale bytes are the same).

One bar differs, the dense pass's layer bar (OUT_RTOL, 4e-3): under fp32 attention / LN an element near an e4m3
midpoint takes the other code, 2^-4 of the element.  Measured (profiles/r21/w_mx48.txt): worst dense layer
error 6.55e-3 here against 4.6e-4 for HPA_FP4 on its own model; DENSE_RTOL is four times the observed worst.
The decode steps keep OUT_RTOL, the K/V rows KV_RTOL."""
import numpy as np
import pytest

import dense_ref64 as dr
from test_gpu_decode_fp4w import _Ref, _model_params, _open
from test_gpu_decode_fp8w import L, P, V
from test_gpu_kv_append import KV_RTOL, OUT_RTOL
from test_gpu_kv_fp8 import _engine_scales

pytestmark = pytest.mark.gpu
DENSE_RTOL = 4 * 6.55e-3
C, NH, F = 128, 2, dr.F


def _engine(hip, B, kv="f32", graph=False):
    m = _open(hip, C, NH, B, kv=hip.HPA_FP8 if kv == "fp8" else hip.HPA_F32, w=hip.HPA_FP4A8, graph=graph)
    if kv == "fp8":
        m.set_kv_scales(*(s[:L] for s in _engine_scales(NH)))
    return m


@pytest.mark.parametrize("kv", ["f32", "fp8"])
def test_prefill_and_decode_steps_against_float64(hip, kv):
    """one ragged prefill (traced), then two traced decode steps, layer by layer against the model"""
    class Ref(_Ref):
        def _a(self, x):  # a layer GEMM's A operand: MXFP8, decode(code) 2^t
            return hip.quantize_mxfp8_rows(np.atleast_2d(x))[2].reshape(np.shape(x))

    lens, pos = dr.ragged_case(70, P)
    dr.case_conditions(lens, pos, P, 5)
    B, R = len(lens), int(lens.sum())
    cfgd, params, deq, groups, _ = _model_params(hip, C, NH)
    m = _engine(hip, B, kv)
    got = m.weight_group_scales()
    assert m.layer_form() == 0 and all(np.array_equal(got[l][i], groups[l][i]) for l in range(L) for i in range(4))
    ref = Ref(cfgd, deq, params)
    rng = np.random.default_rng(C + R)
    tok = rng.integers(0, V, R).astype(np.int32)
    m.fill_random(F, seed=C + R)

    def read(n):  # every layer's rows [0, n[b]); keeps pages: only makes the rows readable
        m.set_positions(n)
        return [[m.read_kv(l, b, int(n[b])) for b in range(B)] for l in range(L)]

    before = read(np.full(B, F))
    m.set_positions(pos)
    xs = m.trace_next_pass(R)
    nxt = m.prefill_ragged(np.split(tok, np.cumsum(lens)[:-1]))
    m.status()
    logits, p1 = m.logits(), pos + lens
    after = read(np.maximum(p1, F))
    dr.check_pass(ref, tok, lens, pos, xs, before, after, KV_RTOL[True], DENSE_RTOL, logits=logits, next_ids=nxt,
                  kv_values=kv != "fp8")
    m.set_positions(p1)
    steps = []
    for s in range(2):
        t = rng.integers(0, V, B).astype(np.int32)
        steps.append((t,) + m.step_traced(t) + (m.logits(),))
    after2 = read(np.maximum(p1 + 2, F))
    m.close()
    for s, (t, ids, x, lg) in enumerate(steps):
        assert np.array_equal(x[0], ref.embed(t, p1 + s))
        for l in range(L):
            want = ref.layer_out(x[l], l, [after2[l][b][0] for b in range(B)], [after2[l][b][1] for b in range(B)], p1 + s + 1)
            assert np.abs(want - x[l + 1]).max() <= OUT_RTOL[True] * np.abs(x[l + 1]).max(), (s, l)
        want, bound = dr.logits64(ref, x[L])
        assert np.all(np.abs(lg - want) <= bound) and np.array_equal(ids, lg.argmax(-1))


@pytest.mark.parametrize("kv", ["f32", "fp8"])
def test_prefill_equals_token_by_token_steps(hip, kv):
    """the same tokens through one prefill (the dense pass and its workspace) and through decode steps: the same
    positions; layer 0's K/V rows bit for bit (a GEMM row and its quantisation never depend on M); deeper rows
    and the logits within twice DENSE_RTOL, the bar each side is held to against the model"""
    B, n = 3, 6
    stream = np.random.default_rng(5).integers(0, V, (n, B)).astype(np.int32)
    steps, pre = _engine(hip, B, kv), _engine(hip, B, kv)
    for m in (steps, pre):
        m.fill_random(F, seed=9)
    for i in range(n):
        steps.step(stream[i])
    pre.prefill_ragged([stream[:, b] for b in range(B)])
    assert np.array_equal(pre.positions(), steps.positions())
    want = steps.logits().astype(np.float64)
    assert np.abs(pre.logits() - want).max() <= 2 * DENSE_RTOL * np.abs(want).max()
    for l, b in np.ndindex(L, B):
        for got, ref in zip(pre.read_kv(l, b, F + n), steps.read_kv(l, b, F + n)):
            assert l > 0 or np.array_equal(got.view(np.int32), ref.view(np.int32))
            assert np.all(np.linalg.norm(got[F:] - ref[F:], axis=-1) <= 2 * DENSE_RTOL * np.linalg.norm(ref[F:], axis=-1))
    steps.close()
    pre.close()


def test_graph_equals_eager(hip):
    """decode steps after a ragged prefill: graph replay == eager bit for bit, five launches per layer"""
    rng = np.random.default_rng(2)
    seqs = [rng.integers(0, V, n).astype(np.int32) for n in (5, 17, 1)]
    eager, graph = _engine(hip, 3), _engine(hip, 3, graph=True)
    for m in (eager, graph):
        m.prefill_ragged(seqs)
    for _ in range(4):
        assert np.array_equal(eager.step(None), graph.step(None))
        assert np.array_equal(eager.logits().view(np.int32), graph.logits().view(np.int32))
    assert eager.layer_form() == graph.layer_form() == 0
    for m in (eager, graph):
        m.close()
