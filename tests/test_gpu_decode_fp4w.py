"""The decode engine on MXFP4 weights (gpt2_decode_init_w, HPA_FP4) against the float64 model of the
dequantised parameters, tests/ref64.Ref64(cfgd, W', w_bf16=True): W' is quantize_mxfp4_rows on the
four layer tensors and quantize_fp8_rows on wte (an fp4 engine keeps wte fp8), all exactly bf16, so
the bf16-weight bars apply as they stand.  The plan, helpers and bars of tests/test_gpu_decode_fp8w.py."""
import numpy as np
import pytest

import dense_ref64 as dr
import ref64
import synth
from test_gpu_decode_fp8w import MATS, L, P, V, _Ref
from test_gpu_kv_append import KV_RTOL, OUT_RTOL
from test_gpu_kv_fp8 import _engine_scales

pytestmark = pytest.mark.gpu

F, MAX_CTX = dr.F, dr.MAX_CTX
_cache = {}


def _model_params(hip, C, NH):
    """(cfgd, params, dequantised params, group-scale bytes [layer][matrix], wte's fp8 scales), one model at a time"""
    if C not in _cache:
        _cache.clear()
        cfgd = dict(maxT=MAX_CTX, V=V, L=L, NH=NH, C=C)
        params = synth.params(cfgd, seed=300 + NH)
        deq, off, sz = params.copy(), synth.offsets(cfgd), synth.sizes(cfgd)
        groups = [[] for _ in range(L)]
        for i, rows in MATS:
            K = sz[i] // (L * rows * C)
            _, sb, Wd = hip.quantize_mxfp4_rows(params[off[i]:off[i] + sz[i]].reshape(L * rows * C, K))
            deq[off[i]:off[i] + sz[i]] = Wd.ravel()
            for l in range(L):
                groups[l].append(sb[l * rows * C:(l + 1) * rows * C])
        _, s_wte, Wd = hip.quantize_fp8_rows(params[:V * C].reshape(V, C))
        deq[:V * C] = Wd.ravel()
        _cache[C] = (cfgd, params, deq, groups, s_wte)
    return _cache[C]


def _open(hip, C, NH, B, kv=None, w=None, graph=False):
    cfgd, params = _model_params(hip, C, NH)[:2]
    m = hip.Model(cfgd, params=params)
    m.decode_init(B, P, MAX_CTX, kv_dtype=hip.HPA_F32 if kv is None else kv, w_dtype=hip.HPA_FP4 if w is None else w)
    m.set_graph(graph)
    return m


@pytest.mark.parametrize("C,NH,kv", [(128, 2, "f32"), (128, 2, "fp8"), (768, 12, "f32")])
def test_prefill_and_decode_steps_against_float64(hip, C, NH, kv):
    """one ragged prefill (traced), then two traced decode steps from where it left the sequences"""
    lens, pos = dr.ragged_case(70, P)
    dr.case_conditions(lens, pos, P, 5)
    B, R = len(lens), int(lens.sum())
    cfgd, params, deq, groups, s_wte = _model_params(hip, C, NH)
    m = _open(hip, C, NH, B, kv=hip.HPA_FP8 if kv == "fp8" else hip.HPA_F32)
    assert m.layer_form() == 0  # five launches per layer
    got = m.weight_group_scales()
    assert all(np.array_equal(got[l][i], groups[l][i]) for l in range(L) for i in range(4))
    assert np.array_equal(m.weight_scales(), np.concatenate([np.ones(L * 9 * C, np.float32), s_wte]))
    if kv == "fp8":
        m.set_kv_scales(*(s[:L] for s in _engine_scales(NH)))
    ref = _Ref(cfgd, deq, params)
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
    assert np.array_equal(m.positions(), pos + lens)
    logits, p1 = m.logits(), pos + lens
    after = read(np.maximum(p1, F))
    # an fp8 pool: the model attends over the rows the pool holds, as tests/test_gpu_dense_pass.py does
    ratios = dr.check_pass(ref, tok, lens, pos, xs, before, after, KV_RTOL[True], OUT_RTOL[True], logits=logits,
                           next_ids=nxt, kv_values=kv != "fp8")
    m.set_positions(p1)
    steps = []
    for s in range(2):
        t = rng.integers(0, V, B).astype(np.int32)
        steps.append((t,) + m.step_traced(t) + (m.logits(),))
    after2 = read(np.maximum(p1 + 2, F))
    m.close()
    refs = [[tuple(np.stack(kv_) for kv_ in zip(*(ref.kv_rows_exact(x[l][b], l) for _, _, x, _ in steps)))
             for b in range(B)] for l in range(L)]
    ratios["step_kv"] = ref64.check_kv(after, after2, p1, np.full(B, 2), ref=refs if kv != "fp8" else None, rtol=KV_RTOL[True])
    for s, (t, ids, x, lg) in enumerate(steps):
        assert np.array_equal(x[0], ref.embed(t, p1 + s))
        for l in range(L):
            want = ref.layer_out(x[l], l, [after2[l][b][0] for b in range(B)], [after2[l][b][1] for b in range(B)], p1 + s + 1)
            r = np.abs(want - x[l + 1]).max() / np.abs(x[l + 1]).max()
            assert r <= OUT_RTOL[True], (s, l, r)
            ratios["step_layer"] = max(ratios.get("step_layer", 0.0), float(r))
        want, bound = dr.logits64(ref, x[L])
        assert np.all(np.abs(lg - want) <= bound) and np.array_equal(ids, lg.argmax(-1))
    print(f"FP4W C={C} kv={kv} " + " ".join(f"{k}={v:.3e}" for k, v in ratios.items()))


def test_graph_equals_eager_and_step_bytes(hip):
    """decode steps after a prefill: graph replay == eager bit for bit; step_bytes is the fp8-weight
    engine's less half a byte per layer weight and its layer scales, plus one byte per 32 layer weights"""
    C, NH, B = 128, 2, 3
    rng = np.random.default_rng(2)
    seqs = [rng.integers(0, V, n).astype(np.int32) for n in (5, 17, 1)]
    eager, graph, f8 = _open(hip, C, NH, B), _open(hip, C, NH, B, graph=True), _open(hip, C, NH, B, w=hip.HPA_FP8)
    for m in (eager, graph, f8):
        m.prefill_ragged(seqs)
    for _ in range(4):
        assert np.array_equal(eager.step(None), graph.step(None))
        assert np.array_equal(eager.logits().view(np.int32), graph.logits().view(np.int32))
        f8.step(None)
    assert eager.layer_form() == graph.layer_form() == 0 and np.array_equal(f8.positions(), eager.positions())
    assert f8.step_bytes()[0] - eager.step_bytes()[0] == L * 12 * C * C // 2 + 4 * L * 9 * C - L * 12 * C * C // 32
    assert f8.step_bytes()[1] == eager.step_bytes()[1]
    with pytest.raises(Exception):
        _open(hip, C, NH, B, kv=3)  # fp4 is a weight format: no such pool
    for m in (eager, graph, f8):
        m.close()


def test_score_and_verify_leave_the_decode_steps_state(hip):
    """score and greedy verify against the same tokens fed through decode steps: the same positions and
    ids; layer 0's K/V rows bit for bit (a GEMM row's sum never depends on M); deeper rows and the
    logits within twice the bf16-weight bars both sides are held to"""
    C, NH, B, n = 128, 2, 3, 6
    first = np.random.default_rng(5).integers(0, V, B).astype(np.int32)
    steps, scored, verified = (_open(hip, C, NH, B) for _ in range(3))
    for m in (steps, scored, verified):
        m.fill_random(F, seed=9)
    stream = np.stack([first] + [steps.step(first if i == 0 else None) for i in range(n)])  # fed ids 0..n-1, then the last pick
    assert np.array_equal(scored.score([stream[:n, b] for b in range(B)])[2], stream[n])
    verified.step(first)  # pending id = stream[1]; drafts: the decode stream's own continuation
    acc, toks, _ = verified.verify([stream[2:n, b].tolist() for b in range(B)])
    assert acc == [n - 2] * B and [t[-1] for t in toks] == stream[n].tolist()
    want = steps.logits().astype(np.float64)
    for m in (scored, verified):
        assert np.array_equal(m.positions(), steps.positions())
        assert np.abs(m.logits() - want).max() <= 2 * OUT_RTOL[True] * np.abs(want).max()
        for l, b in np.ndindex(L, B):
            for got, ref in zip(m.read_kv(l, b, F + n), steps.read_kv(l, b, F + n)):
                assert l > 0 or np.array_equal(got.view(np.int32), ref.view(np.int32))
                assert np.all(np.linalg.norm(got[F:] - ref[F:], axis=-1) <= 2 * KV_RTOL[True] * np.linalg.norm(ref[F:], axis=-1))
    for m in (steps, scored, verified):
        m.close()
