"""The fp8 (OCP e4m3fn) KV pool on the GPU: decode and prefill attention over
fp8 pages, the two covered K/V-append paths (the fused GEMM epilogue; chain
form 6 with the step's first launch), the engine's routing, scales, serving
and capacity.

Attention: the reference sees exactly the values the pool holds (K, V drawn
from U(-1, 1) and passed through round_fp8(., scale); per-head scales 1.0,
0.37 and 2^-3), as the bf16 cases of test_gpu_attention.py do.  Codes decode
exactly and every product and sum is fp32, so the project's 1e-4 max-abs bar
on the attention output carries over.

Engine cases follow tests/test_gpu_kv_append.py (its helpers and ref64 are
imported, neither is changed): 3 layers, MAX_CTX 128, V = 1000,
fill_random(96), ref64.ragged_positions, two traced and two graph-replayed
steps, non-unit scales set through set_kv_scales before fill_random.  Held:
  (a) rows outside [pos, pos + 4) bit-identical to the snapshot;
  (b) rows inside differ from it;
  (c) each appended K/V row against ref64.kv_rows_exact:
      |got - ref| <= KV_RTOL * max|ref row| + half an e4m3 ulp of ref / scale,
      times scale, where ulp(y) = 2^(max(floor(log2 |y|), -6) - 3);
  (d) ref64.layer_out(xs[l], l, K, V, pos + 1) on the pool's own rows against
      xs[l + 1] within OUT_RTOL.
KV_RTOL / OUT_RTOL: 4x the worst ratio measured on the MI355X over these
cases (that module's rule), never above FP32_LAYER_RTOL.  Measured worst
ratios ((c) after the half ulp is taken off; (d)):

  case                                   K/V rows    layer outputs
  C=768 B=20 P=16 auto (chain form 6)    4.98e-08    3.46e-07
  C=768 B=20 P=16 five launches          4.02e-08    6.52e-07
  C=128 B=6  P=32 five launches          0           2.82e-07

The K/V figure is small because the store's half ulp (2^-5 of the value at
worst) absorbs the fp32 GEMM's own error (4e-07 of the row maximum on an fp32
pool, tests/test_gpu_kv_append.py) for all but the elements that sit next to
a rounding boundary.  The other users of the two bounds print their ratios
too; measured: the rescaled step of the graph test 0 (K/V rows), the C = 1280
five-launch step 8.81e-07 and the serving step 2.49e-07 (layer outputs).
"""
import ctypes

import numpy as np
import pytest

import oracle_ctypes as oc
import ref64
import synth
import test_gpu_kv_append as kva
from test_gpu_configs import FP32_LAYER_RTOL
from test_gpu_fused import _run as fused_run

pytestmark = pytest.mark.gpu
TOL = 1e-4
HEAD_SCALES = np.array([1.0, 0.37, 2.0 ** -3], np.float32)
F, MAX_CTX, L = kva.F, kva.MAX_CTX, kva.L

# 4x the measured worst ratios (module docstring), capped by the project's per-layer bar
KV_RTOL = min(4 * 4.98e-8, FP32_LAYER_RTOL)
OUT_RTOL = min(4 * 6.52e-7, FP32_LAYER_RTOL)


@pytest.fixture(scope="module", autouse=True)
def _drop_params():
    yield
    kva._params.clear()


# ---------------------------------------------------------------- attention over fp8 pages
def _pool_case(hip, P, ctxs, NH, rng, kv=None, layers=1):
    """an fp8 pool with per-head scales, pages in a random permutation, K/V = the
    values the pool holds; returns (pool, bt, maxp, ks, vs)"""
    C = NH * 64
    B = len(ctxs)
    maxp = max((c + P - 1) // P for c in ctxs)
    num_pages = B * maxp + 3
    pool = hip.Pool(layers, NH, P, num_pages, dtype=hip.HPA_FP8)
    sc = HEAD_SCALES[np.arange(NH) % 3]
    pool.set_scales(np.tile(sc, (layers, 1)), np.tile(sc[::-1].copy(), (layers, 1)))
    perm = rng.permutation(num_pages).astype(np.int32)
    bt = np.full((B, maxp), -1, np.int32)
    ks, vs, k_next = [], [], 0
    for b, ctx in enumerate(ctxs):
        n = (ctx + P - 1) // P
        bt[b, :n] = perm[k_next:k_next + n]
        k_next += n
        if kv is None:
            k = rng.uniform(-1, 1, (ctx, C)).astype(np.float32)
            v = rng.uniform(-1, 1, (ctx, C)).astype(np.float32)
        else:
            k, v = kv(ctx, C)
        # the values an fp8 pool stores; the oracle sees exactly these
        k = hip.round_fp8(k.reshape(ctx, NH, 64), pool.k_scale[0][None, :, None]).reshape(ctx, C)
        v = hip.round_fp8(v.reshape(ctx, NH, 64), pool.v_scale[0][None, :, None]).reshape(ctx, C)
        pool.write_tokens(0, bt[b, :n], k, v)
        ks.append(k)
        vs.append(v)
    return pool, bt, maxp, ks, vs


def _pages(k, v, ctx, P):
    n = (ctx + P - 1) // P
    C = k.shape[1]
    kp = np.zeros((n * P, C), np.float32)
    vp = np.zeros((n * P, C), np.float32)
    kp[:ctx], vp[:ctx] = k[:ctx], v[:ctx]
    return [kp[i * P:(i + 1) * P].copy() for i in range(n)], [vp[i * P:(i + 1) * P].copy() for i in range(n)]


def _attn_case(hip, P, ctxs, NH, waves=4, seed=0, q_scale=2.0, kv=None, splits=0, repeat=1):
    rng = np.random.default_rng(seed)
    Lb = hip.lib()
    C = NH * 64
    B = len(ctxs)
    pool, bt, maxp, ks, vs = _pool_case(hip, P, ctxs, NH, rng, kv)
    # the write path and the read path agree with the definition: the pool holds exactly ks / vs
    k0, v0 = pool.read_tokens(0, bt[0, :(ctxs[0] + P - 1) // P], ctxs[0])
    assert np.array_equal(k0, ks[0]) and np.array_equal(v0, vs[0])
    q = rng.uniform(-q_scale, q_scale, (B, C)).astype(np.float32)
    pos = np.array([c - 1 for c in ctxs], np.int32)
    d_q = hip.DeviceBuffer.from_array(q)
    d_bt = hip.DeviceBuffer.from_array(bt)
    d_pos = hip.DeviceBuffer.from_array(pos)
    hip.check(Lb.hpa_set_attention_waves(waves))
    try:
        if splits:
            Mp = (B + 15) // 16 * 16
            d_out = hip.DeviceBuffer(Mp * C * 4)
            wsb = Lb.hpa_attn_ws_bytes(B, NH, splits)
            d_ws = hip.DeviceBuffer(max(wsb, 4))
            hip.check(Lb.hpa_memset_async(d_ws.ptr, 0, wsb))
            outs = []
            for _ in range(repeat):
                hip.check(Lb.hpa_paged_attention_decode_split(d_q.ptr, pool.ref, 0, d_bt.ptr, maxp, d_pos.ptr,
                                                              d_out.ptr, B, splits, d_ws.ptr, 1), "split attention")
                hip.check(Lb.hpa_synchronize())
                outs.append(hip.from_frag(d_out.download(Mp * C), B, C))
            for o in outs[1:]:
                assert np.array_equal(o, outs[0])
            cnt = d_ws.download(B * NH, np.int32, offset=B * NH * splits * 68 * 4)
            assert not cnt.any()
            out = outs[0]
        else:
            d_out = hip.DeviceBuffer(q.nbytes)
            hip.check(Lb.hpa_paged_attention_decode(d_q.ptr, pool.ref, 0, d_bt.ptr, maxp, d_pos.ptr, d_out.ptr, B))
            hip.check(Lb.hpa_synchronize())
            out = d_out.download((B, C))
    finally:
        hip.check(Lb.hpa_set_attention_waves(0))
    ref = np.zeros_like(out)
    for b, ctx in enumerate(ctxs):
        kp, vp = _pages(ks[b], vs[b], ctx, P)
        ref[b] = oc.attention_decode(q[b], kp, vp, ctx, NH)
    err = float(np.abs(out - ref).max())
    print(f"FP8ATTN P={P} NH={NH} waves={waves} splits={splits} q={q_scale} err={err:.3e}")
    return out, ref


@pytest.mark.parametrize("P", [16, 32, 64])
def test_fp8_decode_attention_ragged(hip, P):
    out, ref = _attn_case(hip, P, [1, 2, 5, 63, 64, 65, 127, 200, 257, 1024], NH=3, seed=P)
    assert np.abs(out - ref).max() <= TOL


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_fp8_decode_attention_waves(hip, waves):
    out, ref = _attn_case(hip, 16, [1, 70, 333, 1000], NH=2, waves=waves, seed=11)
    assert np.abs(out - ref).max() <= TOL


def test_fp8_decode_attention_peaked_softmax(hip):
    out, ref = _attn_case(hip, 16, [300, 999, 64], NH=2, seed=5, q_scale=40.0)
    assert np.abs(out - ref).max() <= TOL


def test_fp8_decode_attention_all_scores_below_reference_floor(hip):
    """K = 10 everywhere and a hugely negative q: every score < -10000, the
    reference's expsum == 0 branch, output exactly 0"""
    def kv(ctx, C):
        return np.full((ctx, C), 10.0, np.float32), np.ones((ctx, C), np.float32)

    Lb = hip.lib()
    rng = np.random.default_rng(1)
    P, NH, C = 16, 1, 64
    pool, bt, maxp, ks, vs = _pool_case(hip, P, [40, 5], NH, rng, kv)
    q = np.full((2, C), -1000.0, np.float32)
    d_q = hip.DeviceBuffer.from_array(q)
    d_bt = hip.DeviceBuffer.from_array(bt)
    d_pos = hip.DeviceBuffer.from_array(np.array([39, 4], np.int32))
    d_out = hip.DeviceBuffer.from_array(np.ones_like(q))
    hip.check(Lb.hpa_paged_attention_decode(d_q.ptr, pool.ref, 0, d_bt.ptr, maxp, d_pos.ptr, d_out.ptr, 2))
    out = d_out.download((2, C))
    assert np.all(out == 0.0)
    for b, ctx in enumerate((40, 5)):
        kp, vp = _pages(ks[b], vs[b], ctx, P)
        assert np.all(oc.attention_decode(q[b], kp, vp, ctx, NH) == 0.0)


@pytest.mark.parametrize("splits", [2, 4, 16])
def test_fp8_split_context_attention(hip, splits):
    """frag output; three launches bit-identical; the counters read zero afterwards"""
    out, ref = _attn_case(hip, 16, [130, 1000, 64, 700], NH=3, seed=splits, splits=splits, repeat=3)
    assert np.abs(out - ref).max() <= TOL


def test_fp8_prefill_attention(hip):
    """hpa_paged_attention_prefill over fp8 pages against oc.attention_paged on
    the dequantised pages (the oracle attends keys offset .. offset + t, so a
    sequence starting at `start` is its rows start .. start + T - 1 of a
    (start + T)-row pass at offset 0)"""
    Lb = hip.lib()
    rng = np.random.default_rng(20)
    B, T, NH, P = 2, 20, 2, 16
    starts = [0, 37]
    C = NH * 64
    ctxs = [s + T for s in starts]
    pool, bt, maxp, ks, vs = _pool_case(hip, P, ctxs, NH, rng)
    q = rng.uniform(-2, 2, (B * T, C)).astype(np.float32)
    Rp = (B * T + 15) // 16 * 16
    d_q = hip.DeviceBuffer.from_array(q)
    d_bt = hip.DeviceBuffer.from_array(bt)
    d_start = hip.DeviceBuffer.from_array(np.array(starts, np.int32))
    d_out = hip.DeviceBuffer(Rp * C * 4)
    Fp, Ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    hip.check(Lb.hpa_paged_attention_prefill(ctypes.cast(d_q.ptr, Fp), ctypes.addressof(pool.s), 0,
                                             ctypes.cast(d_bt.ptr, Ip), maxp, ctypes.cast(d_start.ptr, Ip), B, T,
                                             ctypes.cast(d_out.ptr, Fp)), "prefill attention")
    hip.check(Lb.hpa_synchronize())
    out = hip.from_frag(d_out.download(Rp * C), B * T, C)
    worst = 0.0
    for b in range(B):
        n, Tb = (ctxs[b] + P - 1) // P, ctxs[b]
        kd, vd = pool.read_tokens(0, bt[b, :n], Tb)  # the dequantised pages
        assert np.array_equal(kd, ks[b]) and np.array_equal(vd, vs[b])
        kpool = np.zeros((n, P, C), np.float32)
        vpool = np.zeros((n, P, C), np.float32)
        kpool.reshape(n * P, C)[:Tb], vpool.reshape(n * P, C)[:Tb] = kd, vd
        inp = np.zeros((1, Tb, 3 * C), np.float32)
        inp[0, starts[b]:, :C] = q[b * T:(b + 1) * T]
        ref = oc.attention_paged(inp, kpool, vpool, list(range(n)), 1, Tb, C, NH, 0, P)[0][0, starts[b]:]
        worst = max(worst, float(np.abs(out[b * T:(b + 1) * T] - ref).max()))
    print(f"FP8PREFILL err={worst:.3e}")
    assert worst <= TOL


# ---------------------------------------------------------------- appends
def _raw(hip, pool):
    """every byte of the pool"""
    out = np.empty(pool.s.bytes, np.uint8)
    hip.check(hip.lib().hpa_memcpy(out.ctypes.data, pool.s.base, out.nbytes), "pool download")
    return out


def test_fp8_append_fused_epilogue_is_exact(hip):
    """one QKV hpa_gemm_fused launch into an fp32 pool and the same launch into
    an fp8 pool: every fp8 byte of the written rows is to_fp8_bits(fp32 value *
    inv), every other byte is unchanged, q is bit-identical.  Head scales 1/512
    (values saturate) and 64 (values land in the subnormal codes)."""
    Lb = hip.lib()
    rng = np.random.default_rng(64)
    NH, P, M = 2, 16, 20
    C = NH * 64
    K, N = C, 3 * C
    npages, maxp = 44, 2
    bt = rng.permutation(npages).astype(np.int32)[:M * maxp].reshape(M, maxp)
    pos = np.array([(5 * r + 3) % (maxp * P) for r in range(M)], np.int32)
    pos[:3] = [0, P - 1, P]
    fixed = dict(x=rng.uniform(-1, 1, (M, K)).astype(np.float32), W=rng.uniform(-0.05, 0.05, (N, K)).astype(np.float32),
                 bias=rng.uniform(-0.1, 0.1, N).astype(np.float32), lw=rng.uniform(0.8, 1.2, K).astype(np.float32),
                 lb=rng.uniform(-0.1, 0.1, K).astype(np.float32))
    scales = np.array([[1.0 / 512, 64.0]], np.float32)
    p32 = hip.Pool(1, NH, P, npages)
    p8 = hip.Pool(1, NH, P, npages, dtype=hip.HPA_FP8)
    p8.set_scales(scales, scales)
    junk = rng.integers(0, 256, p8.s.bytes).astype(np.uint8)
    junk[(junk & 0x7F) == 0x7F] = 0x11  # no NaN codes
    hip.check(Lb.hpa_memcpy(p8.s.base, junk.ctypes.data, junk.nbytes), "pool upload")
    qs = []
    for pool in (p32, p8):
        out, _, _, keep = fused_run(hip, hip.HPA_FEPI_QKV, M, K, N, 8, ln=True, rng=np.random.default_rng(0),
                                    pool_args=(pool, bt, pos), fixed=fixed)
        qs.append(out.download((M, C)))
    assert np.array_equal(qs[0].view(np.uint32), qs[1].view(np.uint32))
    got = _raw(hip, p8)
    want = junk.copy()
    inv = (np.float32(1.0) / scales[0]).astype(np.float32)
    kinds = set()
    for r in range(M):
        k32, v32 = p32.read_tokens(0, bt[r], int(pos[r]) + 1)
        page, slot = int(bt[r, pos[r] // P]), int(pos[r]) % P
        for h in range(NH):
            kc = hip.to_fp8_bits(k32[pos[r], h * 64:(h + 1) * 64] * inv[h])
            vc = hip.to_fp8_bits(v32[pos[r], h * 64:(h + 1) * 64] * inv[h])
            for d in range(64):
                want[Lb.hpa_pool_k_index(p8.ref, 0, page, h, slot, d)] = kc[d]
                want[Lb.hpa_pool_v_index(p8.ref, 0, page, h, slot, d)] = vc[d]
            for c in np.concatenate([kc, vc]) & 0x7F:
                kinds.add("saturated" if c == 0x7E else "subnormal" if 0 < c < 8 else "other")
    assert {"saturated", "subnormal"} <= kinds, kinds
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (len(bad), [(int(i), hex(got[i]), hex(want[i])) for i in bad[:8]])


def _half_ulp_e4m3(y):
    a = np.abs(np.asarray(y, np.float64))
    e = np.maximum(np.floor(np.log2(np.where(a > 0, a, 1.0))), -6.0)
    return np.exp2(e - 3) / 2


def _check_c(after, refs, pos, n, ks, vs):
    """(c): every appended row against its float64 reference; returns the worst
    ratio after the store's half ulp is taken off"""
    worst = 0.0
    for l in range(len(after)):
        if refs[l] is None:
            continue
        for b in range(len(after[l])):
            for wi, sc in enumerate((ks, vs)):
                s = np.repeat(sc[l].astype(np.float64), 64)  # per column
                for j in range(int(n[b])):
                    rr = np.asarray(refs[l][b][wi][j], np.float64)
                    if np.isnan(rr).any():
                        continue
                    got = after[l][b][wi][int(pos[b]) + j].astype(np.float64)
                    assert np.abs(rr / s).max() < 448, "the reference row saturates under this scale"
                    d = np.maximum(np.abs(got - rr) - _half_ulp_e4m3(rr / s) * s, 0.0)
                    ratio = float((d / np.abs(rr).max()).max())
                    worst = max(worst, ratio)
                    assert ratio <= KV_RTOL, (l, b, "KV"[wi], int(pos[b]) + j, ratio)
    return worst


def _engine_scales(NH):
    ks = HEAD_SCALES[(np.arange(L)[:, None] + np.arange(NH)[None, :]) % 3]
    vs = HEAD_SCALES[(np.arange(L)[:, None] + 2 * np.arange(NH)[None, :] + 1) % 3]
    return np.ascontiguousarray(ks), np.ascontiguousarray(vs)


def _open(hip, C, NH, B, P, select, form, w_dtype=None):
    cfgd, params = kva._model_params(C, NH)
    m = hip.Model(cfgd, params=params)
    m.decode_init(B, P, MAX_CTX, kv_dtype=hip.HPA_FP8, w_dtype=hip.HPA_F32 if w_dtype is None else w_dtype)
    if select is not None:
        m.set_layer_kernel(select)
    assert m.layer_form() == form, (m.layer_form(), form)
    return cfgd, params, m


def _check_d(ref, xs, after, pos_next, B):
    worst = 0.0
    for l in range(len(after)):
        out = ref.layer_out(xs[l], l, [after[l][b][0] for b in range(B)], [after[l][b][1] for b in range(B)], pos_next)
        got = xs[l + 1].astype(np.float64)
        r = np.abs(out - got).max(-1) / np.abs(got).max()
        worst = max(worst, float(r.max()))
        assert r.max() <= OUT_RTOL, f"layer {l} sequence {int(r.argmax())}: {r.max():.2e}"
    return worst


def _engine_case(hip, C, NH, B, P, select, form):
    cfgd, params, m = _open(hip, C, NH, B, P, select, form)
    ref = ref64.Ref64(cfgd, params)
    rng = np.random.default_rng(1000 * C + 10 * B + P)
    pos = ref64.ragged_positions(B, P, F)
    ref64.check_position_mix(pos, P)
    ks, vs = _engine_scales(NH)
    m.set_kv_scales(ks, vs)
    gk, gv = m.kv_scales()
    assert np.array_equal(gk, ks) and np.array_equal(gv, vs)
    m.fill_random(F, seed=C + B)
    before = kva._read_all(m, B, np.full(B, F))
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
    assert m.layer_form() == form
    assert np.array_equal(m.positions(), pos + 4)
    n_after = np.maximum(pos + 4, F)
    m.set_positions(n_after)
    after = kva._read_all(m, B, n_after)
    m.close()
    for s in range(2):
        assert np.array_equal(xs[s][0], ref.embed(toks[s], pos + s)), s
    # fill_random: the codes of U(-1, 1) under the scales -- every snapshot value is one the pool can hold
    for l in range(L):
        k, v = before[l][0]
        assert np.array_equal(hip.round_fp8(k.reshape(F, NH, 64), ks[l][None, :, None]).reshape(F, C), k)
        assert np.array_equal(hip.round_fp8(v.reshape(F, NH, 64), vs[l][None, :, None]).reshape(F, C), v)
    refs = []
    for l in range(L):
        k = np.full((4, B, C), np.nan)
        v = np.full((4, B, C), np.nan)
        for s in range(4):
            if s < 2:
                k[s], v[s] = ref.kv_rows_exact(xs[s][l], l)
            elif l == 0:
                k[s], v[s] = ref.kv_rows_exact(ref.embed(toks[s], pos + s), 0)
        refs.append([(k[:, b], v[:, b]) for b in range(B)])
    ref64.check_kv(before, after, pos, np.full(B, 4))  # (a), (b)
    kv_ratio = _check_c(after, refs, pos, np.full(B, 4), ks, vs)
    out_ratio = 0.0
    for s in range(2):
        out_ratio = max(out_ratio, _check_d(ref, xs[s], after, pos + s + 1, B))
    print(f"KVFP8 C={C} NH={NH} B={B} P={P} form={form} kv_ratio={kv_ratio:.3e} out_ratio={out_ratio:.3e}")


@pytest.mark.parametrize("C,NH,B,P,select,form", [
    pytest.param(768, 12, 20, 16, None, 3, id="C768-B20-P16-auto-chain6"),
    pytest.param(768, 12, 20, 16, 0, 0, id="C768-B20-P16-five-launches"),
    pytest.param(128, 2, 6, 32, None, 0, id="C128-B6-P32-five-launches"),
])
def test_fp8_engine_appends(hip, C, NH, B, P, select, form):
    _engine_case(hip, C, NH, B, P, select, form)


def test_fp8_graph_equals_eager_and_scales_need_no_recapture(hip):
    C, NH, B, P = 768, 12, 20, 16
    cfgd, params, m = _open(hip, C, NH, B, P, None, 3)
    ref = ref64.Ref64(cfgd, params)
    ks, vs = _engine_scales(NH)
    m.set_kv_scales(ks, vs)
    pos = ref64.ragged_positions(B, P, F)
    tok = np.random.default_rng(4).integers(0, cfgd["V"], B).astype(np.int32)
    m.fill_random(F, seed=3)
    m.set_positions(pos)
    m.step(tok)
    eager = m.logits()
    m.set_positions(pos)  # the same state: the step rewrites the same rows
    m.set_graph(True)
    m.step(tok)
    m.status()
    assert np.array_equal(eager.view(np.uint32), m.logits().view(np.uint32))
    # other scales, the captured graph kept: the rows follow the new scales
    m.reset()
    ks2, vs2 = (ks * np.float32(0.3)).astype(np.float32), (vs * np.float32(1.7)).astype(np.float32)
    m.set_kv_scales(ks2, vs2)
    m.step(tok)
    m.status()
    assert m.layer_form() == 3
    after = [[m.read_kv(0, b, 1) for b in range(B)]]
    m.close()
    zero = np.zeros(B, np.int32)
    k, v = ref.kv_rows_exact(ref.embed(tok, zero), 0)
    refs = [[(k[b][None], v[b][None]) for b in range(B)]]
    r = _check_c(after, refs, zero, np.ones(B), ks2, vs2)
    print(f"KVFP8 rescaled step kv_ratio={r:.3e}")
    for b in range(B):  # and hold only values the new scales can express
        kk, vv = after[0][b]
        assert np.array_equal(hip.round_fp8(kk.reshape(1, NH, 64), ks2[0][None, :, None]).reshape(1, C), kk)
        assert np.array_equal(hip.round_fp8(vv.reshape(1, NH, 64), vs2[0][None, :, None]).reshape(1, C), vv)
        assert not np.array_equal(hip.round_fp8(kk.reshape(1, NH, 64), ks[0][None, :, None]).reshape(1, C), kk)


# ---------------------------------------------------------------- routing and refusals
def test_fp8_wide_model_runs_five_launches(hip):
    """C = 1280: auto would pick chain form 8, which has no fp8 append"""
    cfgd = dict(maxT=MAX_CTX, V=1000, L=2, NH=20, C=1280)
    params = synth.params(cfgd, seed=720)
    B, P = 4, 16
    m = hip.Model(cfgd, params=params)
    m.decode_init(B, P, MAX_CTX, kv_dtype=hip.HPA_FP8)
    assert m.layer_form() == 0
    for sel in (6, 3, 7):
        m.set_layer_kernel(sel)
        assert m.layer_form() == 0
    m.fill_random(40, seed=2)
    tok = np.arange(B, dtype=np.int32) + 5
    _, xs = m.step_traced(tok)
    m.status()
    after = [[m.read_kv(l, b, 41) for b in range(B)] for l in range(2)]
    m.close()
    r = _check_d(ref64.Ref64(cfgd, params), xs, after, np.full(B, 41), B)
    print(f"KVFP8 C=1280 five launches out_ratio={r:.3e}")


def test_fp8_kv_with_bf16_weights_runs_five_launches(hip):
    cfgd, params = kva._model_params(768, 12)
    m = hip.Model(cfgd, params=params)
    m.decode_init(4, 16, MAX_CTX, kv_dtype=hip.HPA_FP8, w_dtype=hip.HPA_BF16)
    assert m.layer_form() == 0  # never the bf16 chain (4)
    m.set_layer_kernel(1)
    assert m.layer_form() == 0
    m.fill_random(30, seed=1)
    m.step(np.arange(4, dtype=np.int32))
    m.status()
    assert np.isfinite(m.logits()).all()
    assert np.array_equal(m.positions(), np.full(4, 31))
    m.close()


def test_fp8_selected_forms_without_an_fp8_append_fall_to_five_launches(hip):
    cfgd, params = kva._model_params(768, 12)
    m = hip.Model(cfgd, params=params)
    m.decode_init(20, 16, MAX_CTX, kv_dtype=hip.HPA_FP8)
    assert m.layer_form() == 3
    for sel, form in ((6, 0), (3, 0), (7, 0), (5, 3), (0, 0), (1, 3)):
        m.set_layer_kernel(sel)
        assert m.layer_form() == form, (sel, m.layer_form())
    m.close()


def test_fp8_refusals(hip):
    cfgd, params = kva._model_params(128, 2)
    m = hip.Model(cfgd, params=params)
    with pytest.raises(RuntimeError):
        m.decode_init(2, 8, MAX_CTX, kv_dtype=hip.HPA_FP8)  # page size 8
    one = np.ones((L, 2), np.float32)
    m.decode_init(2, 16, MAX_CTX)  # an fp32 engine
    with pytest.raises(RuntimeError):
        m.set_kv_scales(one, one)
    with pytest.raises(RuntimeError):
        m.kv_scales()
    m.decode_init(2, 16, MAX_CTX, kv_dtype=hip.HPA_FP8)
    m.set_kv_scales(one * 0.5, one * 2)
    for bad in (0.0, -1.0, np.nan, np.inf):
        s = one.copy()
        s[1, 1] = bad
        with pytest.raises(RuntimeError):
            m.set_kv_scales(s, one)
        with pytest.raises(RuntimeError):
            m.set_kv_scales(one, s)
    k, v = m.kv_scales()
    assert np.all(k == 0.5) and np.all(v == 2.0)  # a refused call stores nothing
    m.step(np.array([1, 2], np.int32))
    with pytest.raises(RuntimeError):
        m.set_kv_scales(one, one)  # cached codes would change their meaning
    m.reset()
    m.set_kv_scales(one, one)
    m.close()


# ---------------------------------------------------------------- serving, capacity
def test_fp8_serving(hip):
    """ragged prefill, decode steps, release and re-admission on an fp8 pool:
    positions and evictions as on fp32, (d) on the last step"""
    C, NH, B, P = 128, 2, 3, 16
    cfgd, params = kva._model_params(C, NH)
    rng = np.random.default_rng(9)
    seqs = [rng.integers(0, cfgd["V"], n).astype(np.int32) for n in (20, 0, 7)]
    again = [rng.integers(0, cfgd["V"], 5).astype(np.int32), [], []]
    toks = rng.integers(0, cfgd["V"], (3, B)).astype(np.int32)
    ks, vs = _engine_scales(NH)
    trace = {}
    for dt in (hip.HPA_F32, hip.HPA_FP8):
        m = hip.Model(cfgd, params=params)
        m.decode_init(B, P, MAX_CTX, kv_dtype=dt)
        if dt == hip.HPA_FP8:
            m.set_kv_scales(ks, vs)
        log = []
        m.prefill_ragged(seqs)
        log.append((m.positions().tolist(), m.evicted().tolist()))
        for s in range(2):
            m.step(toks[s])
            log.append((m.positions().tolist(), m.evicted().tolist()))
        m.release(0)
        log.append((m.positions().tolist(), m.evicted().tolist()))
        m.prefill_ragged(again)
        log.append((m.positions().tolist(), m.evicted().tolist()))
        pos = m.positions()
        _, xs = m.step_traced(toks[2])
        m.status()
        log.append((m.positions().tolist(), m.evicted().tolist()))
        if dt == hip.HPA_FP8:
            after = [[m.read_kv(l, b, int(pos[b]) + 1) for b in range(B)] for l in range(L)]
            r = _check_d(ref64.Ref64(cfgd, params), xs, after, pos + 1, B)
            print(f"KVFP8 serving out_ratio={r:.3e}")
        m.close()
        trace[dt] = log
    assert trace[hip.HPA_FP8] == trace[hip.HPA_F32]
    assert trace[hip.HPA_FP8][0][0] == [20, 0, 7] and trace[hip.HPA_FP8][-1][0] == [6, 3, 10]


def test_fp8_pool_is_a_quarter_of_the_fp32_pool(hip):
    p32 = hip.Pool(2, 3, 16, 7)
    p8 = hip.Pool(2, 3, 16, 7, dtype=hip.HPA_FP8)
    assert p8.s.elem_bytes == 1 and p8.s.bytes * 4 == p32.s.bytes
    assert p8.s.page_elems == p32.s.page_elems and p8.s.layer_elems == p32.s.layer_elems
    assert p8.s.scales and not p32.s.scales
