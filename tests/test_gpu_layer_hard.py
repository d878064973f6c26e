"""One decode layer of every form against float64, on weights that make the
softmax peaked and at a context where every wave of an attention unit has
work.

The harness is that of tests/test_gpu_kv_append.py (form asserted through
layer_form(), fill_random, ref64.ragged_positions, two traced steps, the
pool's own rows through read_kv, ref64.Ref64.layer_out against xs[l + 1]),
with two changes:

* Weights: synth.params with the Q third of every layer's qkvw (rows 0..C)
  and qkvb multiplied by 10 (25 at C = 128, where 10 leaves the median
  weight of the 5-row case at 0.22: q grows with sqrt(C)).  Scores then have
  a standard deviation of about 3 nats instead of 0.3; asserted on the
  float64 reference over the pool's rows (inputs, no kernel in it): the
  largest softmax weight is >= 0.25 for at least half of the (row, head) pairs of layer 0, and
  E = max_j sum_i |q_i k_ji| / 8 over the keys that carry weight
  (tests/attn_ref64.py) is <= 40 for every pair, so the score-rounding term
  2^-24 E stays under a quarter of FP32_LAYER_RTOL.  The layer output is
  dominated by the attention term: a wrong key is an O(1) relative error.
* Context: fill_random(F = 330) in pools of max_ctx = 384: 6 tiles of 64 keys,
  so each wave of a 4-wave unit has one and some have two; 330 is no multiple
  of 8, 16 or 64.

Bar: the project's FP32_LAYER_RTOL (tests/test_gpu_configs.py), per row and
relative to max|x_{l+1}|, as that module applies it.  bf16 and fp8 pools: K
and V are the rows the pool holds (read_kv); the rows the steps appended are
also held against ref64.kv_rows_exact within FP32_LAYER_RTOL plus half a bf16
ulp (ref64.check_kv) on a bf16 pool; the fp8 case holds its layer outputs to
the bar tests/test_gpu_kv_fp8.py uses for them (OUT_RTOL).  bf16 weights are
out of scope here: the bf16 chain's attention is the stand-alone launch that
tests/test_gpu_attention_hard.py pins.

Requests 2 (the full persistent layer) and 7 (the pipelined halves) carry
their own copies of the attention; they exist in A/B builds only
(XFLAGS=-DHPA_AB) and skip on the product library as tests/test_gpu_layer.py
and tests/test_gpu_pipe.py do.  Request 7 runs every layer in one launch and
cannot be traced: it is held bit for bit to the request-5 step (4 attention
waves, one range) that is held to float64 in the same test.

Measured worst ratios on the MI355X (bar 1e-5; fp8 2.61e-6):

  request, shape, pool                    appended K/V rows   layer outputs
  0  five launches  C=768  B=70 P=16 f32   5.7e-07             1.19e-06
  5  chain form 6   C=768  B=64 P=16 f32   3.8e-07             1.18e-06
  5  chain form 6   C=768  B=33 P=64 f32   5.2e-07             1.05e-06
  5  chain form 6   C=768  B=33 P=8  bf16  1.1e-07             9.8e-07
  5  chain form 6   C=768  B=64 P=32 bf16  1.2e-07             1.11e-06
  6  chain form 8   C=1024 B=17 P=8  f32   6.1e-07             8.9e-07
  3  4-wave chain   C=128  B=5  P=16 f32   2.8e-07             4.9e-07
  5  chain form 6   C=768  B=20 P=16 fp8   -                   9.9e-07
  2  persistent     C=768  B=64 P=16 f32   6.4e-07             1.11e-06   (A/B build)
  2  persistent     C=768  B=17 P=8  f32   5.7e-07             1.43e-06   (A/B build)
  7  pipelined      C=768  B=64 / 17       bit-identical to the request-5 step (A/B build)

(bf16 pools: after the store's half ulp is taken off.)  Median largest
softmax weight 0.39 .. 0.64, largest E 31.2.
"""
import numpy as np
import pytest

import attn_ref64 as ar
import ref64
from test_gpu_configs import FP32_LAYER_RTOL
from test_gpu_kv_fp8 import OUT_RTOL as FP8_OUT_RTOL
from test_gpu_kv_fp8 import _engine_scales

pytestmark = pytest.mark.gpu

F = 330
MAX_CTX = 384
L = 3

_params = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_params():
    yield
    _params.clear()


def _model_params(C, NH):
    cfgd = dict(maxT=MAX_CTX, V=1000, L=L, NH=NH, C=C)
    if C not in _params:
        _params.clear()  # one model at a time
        _params[C] = ar.peaked_params(cfgd, seed=900 + NH)
    return cfgd, _params[C]


def _open(hip, C, NH, B, P, kv_dtype):
    """the engine of a case, initialised: (cfgd, params, model)"""
    cfgd, params = _model_params(C, NH)
    m = hip.Model(cfgd, params=params)
    m.decode_init(B, P, MAX_CTX, kv_dtype=kv_dtype)
    return cfgd, params, m


def _steps(hip, C, NH, B, P, kv, select, form, traced=True, attn_4_waves=False, opener=_open):
    """two steps of a fresh engine from fill_random(F) at ragged positions.
    traced: step_traced (the residual stream entering every layer), else plain
    eager steps.  attn_4_waves: the attention launch as one range of 4 waves.
    opener: what opens and initialises the engine (_open; tests/test_gpu_pool_large.py
    passes one whose pool is large and whose model may have fewer layers).
    Returns (cfgd, params, pos, toks, xs, logits, before, after)."""
    Lb = hip.lib()
    kv_dtype = {"f32": hip.HPA_F32, "bf16": hip.HPA_BF16, "fp8": hip.HPA_FP8}[kv]
    cfgd, params, m = opener(hip, C, NH, B, P, kv_dtype)
    nl = cfgd["L"]
    if select is not None:
        m.set_layer_kernel(select)
    assert m.layer_form() == form, (m.layer_form(), form)
    rng = np.random.default_rng(1000 * C + 10 * B + P)
    pos = ref64.ragged_positions(B, P, F)
    ref64.check_position_mix(pos, P)
    if kv == "fp8":
        m.set_kv_scales(*(s[:nl] for s in _engine_scales(NH)))  # every sequence at position 0
    if attn_4_waves:
        m.set_attn_splits(1)
        hip.check(Lb.hpa_set_attention_waves(4), "waves")
    try:
        m.fill_random(F, seed=C + B)
        before = [[m.read_kv(l, b, F) for b in range(B)] for l in range(nl)]
        m.set_positions(pos)
        toks = rng.integers(0, cfgd["V"], (2, B)).astype(np.int32)
        xs, logits = [], []
        for s in range(2):
            if traced:
                xs.append(m.step_traced(toks[s])[1])
            else:
                m.step(toks[s])
            logits.append(m.logits())
        m.status()
    finally:
        if attn_4_waves:
            hip.check(Lb.hpa_set_attention_waves(0), "waves")
    assert m.layer_form() == form
    assert np.array_equal(m.positions(), pos + 2)
    n_after = np.maximum(pos + 2, F)
    m.set_positions(n_after)  # keeps pages: only makes the rows readable again
    after = [[m.read_kv(l, b, int(n_after[b])) for b in range(B)] for l in range(nl)]
    m.close()
    return cfgd, params, pos, toks, xs, logits, before, after


def _run_case(hip, C, NH, B, P, kv, select, form, attn_4_waves=False, opener=_open):
    cfgd, params, pos, toks, xs, logits, before, after = _steps(hip, C, NH, B, P, kv, select, form,
                                                                attn_4_waves=attn_4_waves, opener=opener)
    nl = cfgd["L"]
    ref = ref64.Ref64(cfgd, params, kv_bf16=kv == "bf16")
    for s in range(2):
        assert np.array_equal(xs[s][0], ref.embed(toks[s], pos + s)), s
    # the inputs are what the module says they are (float64 over the pool's rows)
    wmax, E = ar.input_conditions(ref, xs[0][0], [after[0][b][0] for b in range(B)], [after[0][b][1] for b in range(B)],
                               pos + 1)
    assert np.median(wmax) >= 0.25, float(np.median(wmax))
    assert E.max() <= 40.0, float(E.max())
    # the appended rows: untouched elsewhere, written here, and (fp32 / bf16 pools) equal to float64
    refs = None
    if kv != "fp8":
        refs = []
        for l in range(nl):
            rows = [ref.kv_rows_exact(xs[s][l], l) for s in range(2)]
            refs.append([(np.stack([rows[s][0][b] for s in range(2)]), np.stack([rows[s][1][b] for s in range(2)]))
                         for b in range(B)])
    kv_ratio = ref64.check_kv(before, after, pos, np.full(B, 2), ref=refs, rtol=FP32_LAYER_RTOL, kv_bf16=kv == "bf16")
    # every layer of both steps on the pool's own K/V
    bar = FP8_OUT_RTOL if kv == "fp8" else FP32_LAYER_RTOL
    worst, where = 0.0, None
    for s in range(2):
        for l in range(nl):
            out = ref.layer_out(xs[s][l], l, [after[l][b][0] for b in range(B)], [after[l][b][1] for b in range(B)],
                                pos + s + 1)
            got = xs[s][l + 1].astype(np.float64)
            assert np.isfinite(got).all(), (s, l)
            r = np.abs(out - got).max(-1) / np.abs(got).max()
            if r.max() > worst:
                worst, where = float(r.max()), (s, l, int(r.argmax()), int(pos[r.argmax()]) + s)
    print(f"LAYERHARD C={C} B={B} P={P} kv={kv} select={select} form={form} median_wmax={np.median(wmax):.3f} "
          f"E_max={E.max():.1f} kv_ratio={kv_ratio:.3e} out_ratio={worst:.3e} at (step, layer, seq, pos) {where}")
    assert worst <= bar, f"(step, layer, sequence, position) {where}: {worst:.2e} > {bar:.2e}"
    return logits, after


def _case(C, NH, B, P, kv, select, form):
    return pytest.param(C, NH, B, P, kv, select, form, id=f"req{select}-C{C}-B{B}-P{P}-{kv}")


@pytest.mark.parametrize("C,NH,B,P,kv,select,form", [
    _case(768, 12, 70, 16, "f32", 0, 0),    # five launches, two 64-row groups
    _case(768, 12, 64, 16, "f32", 5, 3),    # chain form 6
    _case(768, 12, 33, 8, "bf16", 5, 3),
    _case(768, 12, 64, 32, "bf16", 5, 3),
    _case(768, 12, 33, 64, "f32", 5, 3),
    _case(1024, 16, 17, 8, "f32", 6, 3),    # chain form 8
    _case(128, 2, 5, 16, "f32", 3, 2),      # the 4-wave chain
    _case(768, 12, 20, 16, "fp8", 5, 3),    # chain form 6 over fp8 pages, scales set at position 0
])
def test_layer_peaked(hip, C, NH, B, P, kv, select, form):
    _run_case(hip, C, NH, B, P, kv, select, form)


def _ab_only(hip, select):
    if not hip.lib().hpa_build_flags() & 1:
        pytest.skip("layer request %d: A/B builds only (-DHPA_AB)" % select)


@pytest.mark.parametrize("C,NH,B,P,kv,select,form", [
    _case(768, 12, 64, 16, "f32", 2, 1), _case(768, 12, 17, 8, "f32", 2, 1),
])
def test_layer_peaked_persistent_layer(hip, C, NH, B, P, kv, select, form):
    """request 2, hpa_layer_units.hip: the full persistent layer carries its own attention units"""
    _ab_only(hip, select)
    _run_case(hip, C, NH, B, P, kv, select, form)


@pytest.mark.parametrize("B,P", [(64, 16), (17, 8)])
def test_layer_peaked_pipelined_halves(hip, B, P):
    """request 7, hpa_pipe.hip: every layer in one launch, so a traced step
    cannot run it (the engine then steps layer by layer through chain form 6).
    Its contract (tests/test_gpu_pipe.py) is bit equality with the request-5
    step whose attention launch is one range of 4 waves.  That step is held to
    float64 here, layer by layer; the pipelined step from the same state must
    then leave the same K/V rows in every layer and the same logits, bit for
    bit -- which carries the float64 pin over to attn_tile / attn_unit."""
    _ab_only(hip, 7)
    C, NH = 768, 12
    ref_logits, ref_after = _run_case(hip, C, NH, B, P, "f32", 5, 3, attn_4_waves=True)
    *_, logits, _, after = _steps(hip, C, NH, B, P, "f32", 7, 5, traced=False)
    for s in range(2):
        assert np.isfinite(logits[s]).all()
        assert np.array_equal(logits[s].view(np.uint32), ref_logits[s].view(np.uint32)), \
            (s, float(np.abs(logits[s] - ref_logits[s]).max()))
    for l in range(L):
        for b in range(B):
            for wi in range(2):
                assert np.array_equal(after[l][b][wi].view(np.uint32), ref_after[l][b][wi].view(np.uint32)), (l, b, "KV"[wi])
