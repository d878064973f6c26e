"""The float64 attention reference (tests/attn_ref64.py) checked against the
arithmetic it stands in for, its case sets and its bar.  CPU only.

The bar of tests/test_gpu_attention_hard.py is set here, from the reference
side alone: REF_WORST is the worst ratio (|got - out| / unit, attn_ref64) of
the reference arithmetic itself -- its sequential fp32 dot, expf and
sequential sums restated in numpy fp32 (attn_ref64.attend_f32), and the
oracle's attention_decode where it is built -- over the decode case sets
(fp32 P = 16, bf16 P = 8, fp8 P = 64) and the prefill case sets of the three
pool dtypes.  Measured worst ratios per kind:

    uniform 0.70   hot 0.49   pair 5.06   ramp_up 2.02   ramp_down 4.81
    below_floor_one 0.00      below_floor_all 0.00 (exactly)
    prefill: uniform 0.94, hot 1.79, pair 4.27; the oracle: pair 5.06

    REF_WORST = 5.1        BAR = 8 x REF_WORST = 40.8 units

The factor 8 is for what the kernels do differently from the reference: tree
and strided summation orders, the hardware exp2 with log2(e) folded into the
scale, and the fp8 path's scales applied after the sums.  No kernel's result
enters either number.

Every mutation of attn_ref64.MUTATIONS -- a key dropped at either end, the
neighbour read at a tile edge, the running max started at -inf, the
accumulator not rescaled when the max rises, a stale slot weighted by 0
instead of excluded -- exceeds BAR on at least one case, while the unmutated
online form stays within REF_WORST's order.
"""
import numpy as np
import pytest

import attn_ref64 as ar
from pagedattn import HPA_BF16, HPA_F32, HPA_FP8

REF_WORST = 5.1
BAR = 8 * REF_WORST

DECODE_SETS = ((16, HPA_F32), (8, HPA_BF16), (64, HPA_FP8))
_cache = {}


def _decode(P, dtype):
    if ("d", P, dtype) not in _cache:
        _cache["d", P, dtype] = ar.decode_cases(P, dtype)
    return _cache["d", P, dtype]


def _prefill(dtype):
    if ("p", dtype) not in _cache:
        _cache["p", dtype] = ar.prefill_cases(dtype)
    return _cache["p", dtype]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def _restated(cs):
    got = np.zeros((len(cs.seq), ar.C), np.float32)
    for si, (K, V) in enumerate(cs.seqs):
        rows = np.nonzero(cs.seq == si)[0]
        for h in range(ar.NH):
            c = slice(h * ar.HS, (h + 1) * ar.HS)
            if rows.size:
                got[rows, c] = ar.attend_f32(cs.q[rows, c], K[:, c], V[:, c], cs.ctx[rows])
    return got


@pytest.mark.parametrize("P,dtype", DECODE_SETS)
def test_reference_arithmetic_within_ref_worst_decode(P, dtype):
    cs = _decode(P, dtype)
    r = cs.ratios(_restated(cs))
    by = cs.worst_by_kind(r)
    print(f"ATTNREF decode P={P} dtype={dtype} rows={len(cs.seq)} " + " ".join(f"{k}={v:.3f}" for k, v in by.items()))
    assert set(by) == set(ar.KINDS)
    assert r.max() <= REF_WORST, by
    assert by["below_floor_all"] == 0.0


@pytest.mark.parametrize("dtype", [HPA_F32, HPA_BF16, HPA_FP8])
def test_reference_arithmetic_within_ref_worst_prefill(dtype):
    cs = _prefill(dtype)
    r = cs.ratios(_restated(cs))
    print(f"ATTNREF prefill dtype={dtype} rows={len(cs.seq)} "
          + " ".join(f"{k}={v:.3f}" for k, v in cs.worst_by_kind(r).items()))
    assert r.max() <= REF_WORST


def test_oracle_attention_decode_within_ref_worst():
    """the C oracle's own attention over the fp32 decode set (skipped only where the oracle is not built)"""
    oc = pytest.importorskip("oracle_ctypes")
    try:
        oc.lib()
    except (OSError, RuntimeError) as e:
        pytest.skip(f"oracle not built: {e}")
    P = 16
    cs = _decode(P, HPA_F32)
    pages = []
    for K, V in cs.seqs:
        n = (K.shape[0] + P - 1) // P
        kp, vp = np.zeros((n * P, ar.C), np.float32), np.zeros((n * P, ar.C), np.float32)
        kp[:K.shape[0]], vp[:K.shape[0]] = K, V
        pages.append(([kp[i * P:(i + 1) * P].copy() for i in range(n)], [vp[i * P:(i + 1) * P].copy() for i in range(n)]))
    got = np.stack([oc.attention_decode(cs.q[i], *pages[cs.seq[i]], int(cs.ctx[i]), ar.NH) for i in range(len(cs.seq))])
    r = cs.ratios(got)
    print("ATTNREF oracle " + " ".join(f"{k}={v:.3f}" for k, v in cs.worst_by_kind(r).items()))
    assert r.max() <= REF_WORST


def _online(cs, mutate, kinds=None, stale=False):
    """attend_online over the rows of cs (optionally only some kinds); stale:
    K, V padded to whole 64-key tiles with NaN rows, as a poisoned pool holds them"""
    got = np.zeros((len(cs.seq), ar.C))
    for i in range(len(cs.seq)):
        K, V = cs.seqs[cs.seq[i]]
        if stale:
            pad = np.full((-K.shape[0] % 64, ar.C), np.nan)
            K, V = np.concatenate([K, pad]), np.concatenate([V, pad])
        for h in range(ar.NH):
            if kinds is not None and cs.kind[i][h] not in kinds:
                got[i, h * ar.HS:(h + 1) * ar.HS] = cs.reference()[0][i, h * ar.HS:(h + 1) * ar.HS]
                continue
            c = slice(h * ar.HS, (h + 1) * ar.HS)
            got[i, c] = ar.attend_online(cs.q[i, c], K[:, c], V[:, c], int(cs.ctx[i]), mutate)
    return got


def test_online_form_unmutated_within_bar():
    """the tile-wise form on NaN-padded pages: finite and within the bar (a select, not a product, masks the slots)"""
    cs = _decode(16, HPA_F32)
    r = cs.ratios(_online(cs, None, stale=True))
    assert r.max() <= REF_WORST, cs.worst_by_kind(r)


@pytest.mark.parametrize("mutate", ar.MUTATIONS)
def test_mutations_exceed_the_bar(mutate):
    cs = _decode(16, HPA_F32)
    r = cs.ratios(_online(cs, mutate, stale=True))
    by = cs.worst_by_kind(r)
    print(f"ATTNREF mutation {mutate}: " + " ".join(f"{k}={v:.3g}" for k, v in by.items()))
    assert r.max() > BAR, by
    caught_by = {"drop_last": "hot", "drop_first": "hot", "next_at_tile_edge": "hot",
                 "max_from_minus_inf": "below_floor_all", "no_alpha": "ramp_up", "stale_times_zero": "uniform"}[mutate]
    assert by[caught_by] > BAR, by  # the case built for it
    if mutate == "stale_times_zero":
        assert np.isinf(r).any()  # NaN got: reported as an infinite ratio


def test_prefill_set_catches_a_dropped_own_key():
    """a prefill row that loses its own key (the last it sees) or key 0 exceeds the bar"""
    cs = _prefill(HPA_F32)
    for mutate in ("drop_last", "drop_first"):
        assert cs.ratios(_online(cs, mutate)).max() > BAR


def test_band_assertion():
    rng = np.random.default_rng(0)
    V = rng.uniform(-1, 1, (3, 64))
    K = np.zeros((3, 64))
    K[:, 0] = [0.0, -90.0 * 8, -130.0 * 8]
    q = np.zeros(64)
    q[0] = 1.0
    with pytest.raises(ar.BandError):
        ar.attend(q, K, V)
    K[1, 0] = -79.0 * 8
    r = ar.attend(q, K, V)
    assert np.isfinite(r.out).all()
    # <= -120 is exactly 0: the output does not see key 2 at all
    V2 = V.copy()
    V2[2] = 1e30
    assert np.array_equal(ar.attend(q, K, V2).out, r.out)


def test_floor_rule():
    """every score below -10000: p relative to the floor; far below: exactly 0 output, unit only the denormal term"""
    V = np.ones((2, 64))
    K = np.zeros((2, 64))
    K[:, 0] = [-10050.0 * 8, -10400.0 * 8]
    q = np.zeros(64)
    q[0] = 1.0
    r = ar.attend(q, K, V)
    assert np.allclose(r.out, 1.0) and r.E[0] == 10050.0
    K[0, 0] = -10200.0 * 8
    r = ar.attend(q, K, V)
    assert not r.out.any() and r.E[0] == 0.0 and np.all(r.unit == 2 * 2.0 ** -126)


def test_positions():
    # S = 1, 4 waves, ctx 1000 (16 tiles): the waves' last tiles are 12..15
    p = ar.positions(1000, 16, 4, 1)
    assert set(p) >= {0, 1, 15, 16, 62, 63, 64, 65, 998, 999, 768, 831, 832, 895, 896, 959, 960}
    assert all(0 <= j < 1000 for j in p) and p == sorted(set(p))
    # 3 ranges of 16 tiles: it0 = 0, 5, 10
    assert ar.tile_ranges(1024, 3) == [(0, 5), (5, 10), (10, 16)]
    p = ar.positions(1024, 8, 8, 3)
    assert set(p) >= {319, 320, 639, 640, 7, 8, 1022, 1023}
    # S = 16 on a short context: ranges with no tile, positions stay inside
    assert ar.tile_ranges(65, 16)[:8] == [(0, 0)] * 7 + [(0, 1)]
    assert ar.positions(1, 64, 2, 16) == [0]
    assert ar.positions(2, 8, 1, 1) == [0, 1]
    for ctx in ar.CONTEXTS:
        for NW, S in ar.LAUNCHES:
            p = ar.positions(ctx, 16, NW, S)
            assert p[0] == 0 and p[-1] == ctx - 1
            r = ar.tile_ranges(ctx, S)
            assert r[0][0] == 0 and r[-1][1] == (ctx + 63) // 64 and all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert ar.prefill_hot_choices(70, 20) == [0, 63, 64, 69, 70, 79, 80, 89, 90]
    assert ar.prefill_hot_choices(0, 0) == [0]


def test_case_sets_cover_what_they_claim():
    cs = _decode(16, HPA_F32)
    out, unit, E, wmax = cs.reference()
    kinds = np.array(cs.kind)
    assert set(cs.ctx.tolist()) == set(ar.CONTEXTS)
    assert (wmax[kinds == "hot"] > 0.99).all()          # the hot key wins by tens of nats
    assert (wmax[(kinds == "pair")] < 1.0 - 1e-6).any()  # pairs share the weight
    long_uniform = (kinds == "uniform") & (cs.ctx >= 128)[:, None]
    assert long_uniform.sum() >= 6 * ar.NH and (wmax[long_uniform] < 0.5).all()
    assert not out[np.repeat(kinds == "below_floor_all", ar.HS, 1)].any()
    one = np.repeat(kinds == "below_floor_one", ar.HS, 1)
    assert np.abs(out[one]).max() > 0.5 and (wmax[kinds == "below_floor_one"] > 1.0 - 1e-12).all()
    # every hot position of every launch is some row's hot key
    for ctx in (65, 1000):
        su = [i for i in range(len(cs.seq)) if cs.ctx[i] == ctx and cs.kind[i][0] == "hot"]
        K = cs.seqs[cs.seq[su[0]]][0]
        aimed = set()
        for i in su:
            for h in range(ar.NH):
                c = slice(h * ar.HS, (h + 1) * ar.HS)
                aimed.add(int(np.argmax(K[:, c] @ cs.q[i, c])))
        assert aimed == set(ar.launch_positions(ctx, 16))


def test_peaked_weights_make_a_wrong_key_an_o1_layer_error():
    """the engine-level inputs of tests/test_gpu_layer_hard.py, on a stand-in
    pool (K, V ~ U(-1, 1), as fill_random draws them): the asserted input
    conditions hold, and a layer that reads the neighbour of a row's heaviest
    key leaves the float64 layer output by an O(1) fraction of max|x|, five
    orders above the per-layer bar"""
    import ref64
    from test_gpu_configs import FP32_LAYER_RTOL
    cfgd = dict(maxT=384, V=1000, L=1, NH=2, C=128)
    B, P, F = 12, 16, 330
    rng = np.random.default_rng(5)
    pos = ref64.ragged_positions(B, P, F)
    tok = rng.integers(0, cfgd["V"], B)
    K = [rng.uniform(-1, 1, (p + 1, cfgd["C"])).astype(np.float32) for p in pos]
    V = [rng.uniform(-1, 1, (p + 1, cfgd["C"])).astype(np.float32) for p in pos]
    ref = ref64.Ref64(cfgd, ar.peaked_params(cfgd, seed=902))
    x0 = ref.embed(tok, pos)
    wmax, E = ar.input_conditions(ref, x0, K, V, pos + 1)
    assert np.median(wmax) >= 0.25 and E.max() <= 40.0, (float(np.median(wmax)), float(E.max()))
    good = ref.layer_out(x0, 0, K, V, pos + 1)
    q = ref._qkv(x0, 0, 0, ref.C)
    rows = np.nonzero(pos >= 1)[0]
    V2 = [v.copy() for v in V]
    for b in rows:  # the heaviest key's V row replaced by its neighbour's
        for h in range(ar.NH):
            c = slice(h * ar.HS, (h + 1) * ar.HS)
            j = int(np.argmax(K[b][:, c].astype(np.float64) @ q[b, c]))
            V2[b][j, c] = V[b][j + 1 if j + 1 <= pos[b] else j - 1, c]
    moved = np.abs(ref.layer_out(x0, 0, K, V2, pos + 1) - good).max(-1)[rows] / np.abs(good).max()
    print(f"ATTNREF layer sensitivity: neighbour of the heaviest key: min {moved.min():.2e} median {np.median(moved):.2e}")
    assert moved.min() > 1e4 * FP32_LAYER_RTOL
