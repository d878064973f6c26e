"""The K/V pages every decode path appends, read back and pinned at ragged
per-sequence positions.

The engine has six K/V-append implementations (the fused QKV epilogue of
hpa_gemm_fused, the 4-wave chain, chain form 6 and its first launch, chain
form 8, the bf16-weight chain and its first launch), each templated on page
size and pool dtype.  Every case here runs one of them -- asserting
model.layer_form() so it cannot quietly test another -- on a 3-layer model of
a real width (first launch, a middle chain launch, the last chain launch)
whose sequences sit at different positions: 0, P-1 (the next step opens page
1), P, F-3, F (as fill_random(F = 96) left it: where P divides F its first
step needs a page the manager has not handed out yet; 96 is no multiple of
64, so at P = 64 that row lands mid-page), else (7 b + 3 (b // 16)) % (F - 3).
pos % P then takes at least 4 values in every 16-row block of 6 or more rows
(asserted; ref64.check_position_mix says why a 5-row batch cannot reach 4),
so an epilogue lane that took the position, the page or the wpe row of a
neighbouring row of its block fails here.

One case: snapshot every layer's rows [0, F) of every sequence, lower the
positions, two eager traced steps and two graph-replayed steps with random
tokens, status(), then read everything again and hold (tests/ref64.py):
  (a) every row outside [pos, pos + 4) is bit-identical to the snapshot;
  (b) every (row, head) inside differs from it (rows past F have no snapshot);
  (c) every row inside equals the float64 reference: from the traced residual
      stream on every layer (traced steps), from wte[tok] + wpe[pos] on layer
      0 (graph steps);
  xs[0] == wte[tok] + wpe[pos] exactly (the ragged wpe lookup);
  ref64.layer_out(xs[l], l, K, V, pos + 1) against xs[l + 1], K and V being
  the pool's own rows: the per-layer pin at ragged positions against float64.

Tolerances: |got - ref| <= rtol * max|ref row| per K/V row (+ half a bf16 ulp
of the reference in a bf16 pool), rtol * max|x_{l+1}| per layer output.  rtol
is 4x the worst ratio measured on the MI355X over all cases of the numeric
mode (run-to-run headroom; forms and summation orders will change), never
above the project's per-layer bars FP32_LAYER_RTOL / BF16_LAYER_RTOL
(tests/test_gpu_configs.py).  Measured worst ratios:

  numeric mode    K/V rows                            layer outputs
  fp32 weights    1.17e-06 (form 8, C=1280 B=64 P=64)  1.24e-06 (five launches, C=1600 B=20)
  bf16 weights    1.61e-04 (bf16 chain, B=200 P=8)     2.12e-03 (bf16 chain, B=200 P=8)

(fp32 weights, other forms: chain form 6 4.2e-07 / 3.9e-07, the 4-wave chain
3.2e-07 / 2.3e-07, ragged prefill 4.1e-07 on K/V rows; bf16 weights: five
launches 1.5e-04 / 1.7e-03, ragged prefill 3.5e-05.)  4x the bf16-weights
layer figure is 8.5e-03, above BF16_LAYER_RTOL, so that bar is the project's
4e-3 itself; the other three are 4x the measurement.

Pages owned by no sequence cannot be read through the model API, so a stray
store into a free page stays unchecked.
"""
import numpy as np
import pytest

import ref64
import synth
from pagedattn import round_bf16
from test_gpu_configs import BF16_LAYER_RTOL, FP32_LAYER_RTOL

pytestmark = pytest.mark.gpu

F = 96          # fill_random context
MAX_CTX = 128   # maxT = max_ctx
L = 3

# 4x the measured worst ratios (module docstring), capped by the project's per-layer bars
KV_RTOL = {False: min(4 * 1.17e-6, FP32_LAYER_RTOL), True: min(4 * 1.61e-4, BF16_LAYER_RTOL)}  # keyed by w_bf16
OUT_RTOL = {False: min(4 * 1.24e-6, FP32_LAYER_RTOL), True: min(4 * 2.12e-3, BF16_LAYER_RTOL)}

_params = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_params():
    yield
    _params.clear()


def _model_params(C, NH):
    cfgd = dict(maxT=MAX_CTX, V=1000, L=L, NH=NH, C=C)
    if C not in _params:
        for wide in [c for c in _params if c >= 1024]:  # one wide model at a time (C = 1600 is 95 M parameters)
            del _params[wide]
        _params[C] = synth.params(cfgd, seed=700 + NH)
    return cfgd, _params[C]


def _open(hip, C, NH, B, P, kv_bf16, w_bf16, select, form):
    cfgd, params = _model_params(C, NH)
    m = hip.Model(cfgd, params=params)
    m.decode_init(B, P, MAX_CTX, kv_dtype=hip.HPA_BF16 if kv_bf16 else hip.HPA_F32,
                  w_dtype=hip.HPA_BF16 if w_bf16 else hip.HPA_F32)
    if select is not None:
        m.set_layer_kernel(select)
    assert m.layer_form() == form, (m.layer_form(), form)
    return cfgd, params, m


def _read_all(m, B, n, nl=L):
    return [[m.read_kv(l, b, int(n[b])) for b in range(B)] for l in range(nl)]


def _run_case(hip, C, NH, B, P, kv_bf16, w_bf16, select, form, opener=_open):
    """opener: what opens and initialises the engine (_open; tests/test_gpu_pool_large.py
    passes one whose pool is large and whose model may have fewer layers)"""
    cfgd, params, m = opener(hip, C, NH, B, P, kv_bf16, w_bf16, select, form)
    nl = cfgd["L"]
    ref = ref64.Ref64(cfgd, params, w_bf16=w_bf16, kv_bf16=kv_bf16)
    rng = np.random.default_rng(1000 * C + 10 * B + P)
    pos = ref64.ragged_positions(B, P, F)
    ref64.check_position_mix(pos, P)
    m.fill_random(F, seed=C + B)
    before = _read_all(m, B, np.full(B, F), nl)
    m.set_positions(pos)
    toks = rng.integers(0, cfgd["V"], (4, B)).astype(np.int32)
    xs = []
    for s in range(2):
        _, x = m.step_traced(toks[s])
        xs.append(x)
    m.set_graph(True)
    for s in range(2, 4):
        m.step(toks[s])
    m.status()
    assert np.array_equal(m.positions(), pos + 4)
    n_after = np.maximum(pos + 4, F)
    m.set_positions(n_after)  # keeps pages: only makes the rows readable again
    after = _read_all(m, B, n_after, nl)
    m.close()

    # the ragged wpe lookup, exact
    for s in range(2):
        assert np.array_equal(xs[s][0], ref.embed(toks[s], pos + s)), s
    # reference rows: traced steps on every layer, graph steps on layer 0
    refs = []
    for l in range(nl):
        k = np.full((4, B, C), np.nan)
        v = np.full((4, B, C), np.nan)
        for s in range(4):
            if s < 2:
                k[s], v[s] = ref.kv_rows_exact(xs[s][l], l)
            elif l == 0:
                k[s], v[s] = ref.kv_rows_exact(ref.embed(toks[s], pos + s), 0)
        refs.append([(k[:, b], v[:, b]) for b in range(B)])
    kv_ratio = ref64.check_kv(before, after, pos, np.full(B, 4), ref=refs, rtol=KV_RTOL[w_bf16], kv_bf16=kv_bf16)
    # every layer of the traced steps on the pool's own K/V
    out_ratio = 0.0
    for s in range(2):
        for l in range(nl):
            out = ref.layer_out(xs[s][l], l, [after[l][b][0] for b in range(B)], [after[l][b][1] for b in range(B)],
                                pos + s + 1)
            got = xs[s][l + 1].astype(np.float64)
            r = np.abs(out - got).max(-1) / np.abs(got).max()
            out_ratio = max(out_ratio, float(r.max()))
            assert r.max() <= OUT_RTOL[w_bf16], (f"step {s} layer {l} sequence {int(r.argmax())} "
                                                f"(position {int(pos[r.argmax()]) + s}): {r.max():.2e}")
    print(f"KVREF C={C} NH={NH} B={B} P={P} kv_bf16={int(kv_bf16)} w_bf16={int(w_bf16)} form={form} "
          f"kv_ratio={kv_ratio:.3e} out_ratio={out_ratio:.3e}")


def _case(C, NH, B, P, pool):
    return pytest.param(C, NH, B, P, pool == "bf16", id=f"C{C}-B{B}-P{P}-{pool}")


@pytest.mark.parametrize("C,NH,B,P,kv_bf16", [_case(768, 12, 64, 16, "f32"), _case(768, 12, 33, 8, "bf16"),
                                              _case(768, 12, 5, 64, "f32"), _case(768, 12, 17, 32, "bf16")])
def test_chain_form6_and_first_launch(hip, C, NH, B, P, kv_bf16):
    _run_case(hip, C, NH, B, P, kv_bf16, False, select=5, form=3)


@pytest.mark.parametrize("C,NH,B,P,kv_bf16", [_case(1024, 16, 17, 8, "bf16"), _case(1280, 20, 64, 64, "f32"),
                                              _case(1600, 25, 33, 32, "f32"), _case(768, 12, 8, 16, "bf16")])
def test_chain_form8(hip, C, NH, B, P, kv_bf16):
    _run_case(hip, C, NH, B, P, kv_bf16, False, select=6, form=3)


@pytest.mark.parametrize("C,NH,B,P,kv_bf16", [_case(128, 2, 5, 16, "f32"), _case(128, 2, 21, 8, "bf16")])
def test_chain_4wave(hip, C, NH, B, P, kv_bf16):
    """the only persistent form a C = 128 model runs: the engine's default there"""
    _run_case(hip, C, NH, B, P, kv_bf16, False, select=None, form=2)


@pytest.mark.parametrize("C,NH,B,P,kv_bf16", [_case(768, 12, 70, 16, "f32"), _case(1600, 25, 20, 32, "f32")])
def test_five_launches(hip, C, NH, B, P, kv_bf16):
    """hpa_gemm_fused's QKV epilogue: two 64-row groups at B = 70; the ring /
    stream-K qkv at XL width"""
    _run_case(hip, C, NH, B, P, kv_bf16, False, select=0, form=0)


@pytest.mark.parametrize("C,NH,B,P,kv_bf16", [_case(768, 12, 1, 16, "f32"), _case(768, 12, 40, 8, "bf16"),
                                              _case(768, 12, 200, 8, "bf16")])
def test_bf16_chain_and_first_launch(hip, C, NH, B, P, kv_bf16):
    _run_case(hip, C, NH, B, P, kv_bf16, True, select=None, form=4)


def test_bf16_five_launches(hip, monkeypatch):
    """bf16 weights on the five-launch loop (as test_config5_layer_pinned_full_batch selects it)"""
    monkeypatch.setenv("HPA_LAYER_KERNEL", "0")
    _run_case(hip, 768, 12, 96, 8, True, True, select=None, form=0)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16_weights_and_pool"])
def test_prefill_ragged_appends(hip, bf16):
    """prefill_ragged of 0, 1, 17 and 40 tokens from ragged positions (C = 768,
    B = 4, P = 16): (a)/(b) on every layer, (c) from the embedding where no
    trace is needed; the untouched sequence's rows bit-identical.  (c) on every
    layer, the layer outputs and the decode rows of the dense pass are held
    through its trace by tests/test_gpu_dense_pass.py"""
    C, NH, B, P = 768, 12, 4, 16
    cfgd, params, m = _open(hip, C, NH, B, P, bf16, bf16, None, 4 if bf16 else 3)
    ref = ref64.Ref64(cfgd, params, w_bf16=bf16, kv_bf16=bf16)
    lens = np.array([0, 1, 17, 40])
    pos = np.array([F - 3, P - 1, P, 7], np.int32)  # 17 tokens fill page 1 and open page 2; 40 start mid-page
    rng = np.random.default_rng(77)
    seqs = [rng.integers(0, cfgd["V"], n).astype(np.int32) for n in lens]
    m.fill_random(F, seed=5)
    before = _read_all(m, B, np.full(B, F))
    m.set_positions(pos)
    m.prefill_ragged(seqs)
    m.status()
    assert np.array_equal(m.positions(), pos + lens)
    m.set_positions(np.full(B, F, np.int32))
    after = _read_all(m, B, np.full(B, F))
    m.close()
    refs = [[ref.kv_rows_exact(ref.embed(seqs[b], pos[b] + np.arange(lens[b])), 0) for b in range(B)], None, None]
    ratio = ref64.check_kv(before, after, pos, lens, ref=refs, rtol=KV_RTOL[bf16], kv_bf16=bf16)
    for l in range(L):
        for wi in range(2):
            assert np.array_equal(before[l][0][wi], after[l][0][wi])
    print(f"KVREF prefill bf16={int(bf16)} kv_ratio={ratio:.3e}")


def test_bf16_pool_rows_are_rne_of_fp32_pool_rows(hip):
    """chain form 6's first launch (768, 12, 33, 8): qkv(0)'s arithmetic does
    not depend on the pool dtype, so from the same tokens and positions the
    rows layer 0 appends to a bf16 pool are round-to-nearest-even of the rows
    it appends to an fp32 pool, bit for bit (one eager and one graph step)"""
    C, NH, B, P = 768, 12, 33, 8
    pos = ref64.ragged_positions(B, P, F)
    toks = np.random.default_rng(3).integers(0, 1000, (2, B)).astype(np.int32)
    rows = []
    for kv_bf16 in (False, True):
        cfgd, params, m = _open(hip, C, NH, B, P, kv_bf16, False, 5, 3)
        m.fill_random(F, seed=8)
        m.set_positions(pos)
        m.step(toks[0])
        m.set_graph(True)
        m.step(toks[1])
        m.status()
        n = np.maximum(pos + 2, F)
        m.set_positions(n)
        kv = [m.read_kv(0, b, int(n[b])) for b in range(B)]
        m.close()
        rows.append([(k[pos[b]:pos[b] + 2], v[pos[b]:pos[b] + 2]) for b, (k, v) in enumerate(kv)])
    for b in range(B):
        for wi, w in enumerate("KV"):
            want = round_bf16(rows[0][b][wi])
            got = rows[1][b][wi]
            assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), \
                (b, w, int(pos[b]), float(np.abs(want - got).max()))
