"""tests/ref64.py on the CPU: the float64 layer reference against the pinned
oracle, and the K/V-append checker against injected faults.

Reference against the oracle (C=128, L=2, NH=2, B=3, page 8, 40 decode steps
at ragged positions): the float64 decoder's own residual stream, rounded to
fp32 at every layer boundary, is fed to oracle.PagedDecoder.step_forced, so
both sides run every layer from identical inputs.  Compared per step and
layer: ref64.kv_rows against the row the oracle appended (read back through
oracle_paged_get_kv), and ref64.layer_out -- on the oracle's own cache --
against the oracle's layer output.  Bars are the project's per-layer ones
(tests/test_gpu_configs.py): 1e-5 x max|x| with fp32 weights,
BF16_LAYER_RTOL x max|x| with bf16 weights; a bf16 pool adds half a bf16 ulp
of the reference to a K/V element.

Worst ratios measured (this file, x86-64, numpy float64):

  mode                 K/V rows     layer outputs
  fp32                 8.1e-07      9.1e-07
  kv_bf16              8.5e-08      1.0e-06
  w_bf16 + kv_bf16     3.3e-08      6.2e-05

(the K/V figure of a bf16 pool is what is left after the half ulp; the fp32
figures are the oracle's sequential fp32 sums; the bf16-weights layer figure
is single bf16-ulp flips of GEMM inputs that the two sides computed a few
fp32 ulps apart.)

Checker self-test: "GPU results" are the float64 reference rounded to fp32
(and to bf16 for a bf16 pool) on three sequences at ragged positions; the
clean result passes, and each injected fault -- a row at slot +/- 1, a row in
the next sequence's page, K and V swapped for a head, a head's two 32-dim
halves swapped, a row computed from its neighbour's position, a bf16 element
truncated, a stray store before the position, an expected row left unwritten
-- fails with its layer, sequence, position, head and K-or-V named.
"""
import copy

import numpy as np
import pytest

import oracle_ctypes as oc
import ref64
import synth
from pagedattn import from_bf16_bits, round_bf16
from test_gpu_configs import BF16_LAYER_RTOL, FP32_LAYER_RTOL

SMALL = dict(maxT=128, V=1000, L=2, NH=2, C=128)
C, L, NH = SMALL["C"], SMALL["L"], SMALL["NH"]


@pytest.fixture(scope="module")
def params():
    return synth.params(SMALL, seed=11)


@pytest.mark.parametrize("w_bf16,kv_bf16", [(False, False), (False, True), (True, True)],
                         ids=["fp32", "kv_bf16", "w_bf16_kv_bf16"])
def test_ref64_matches_oracle(params, w_bf16, kv_bf16):
    B, P, steps = 3, 8, 40
    start = [0, 5, 23]  # ragged: every step has three different slots in flight
    rtol = BF16_LAYER_RTOL if w_bf16 else FP32_LAYER_RTOL
    ref = ref64.Ref64(SMALL, params, w_bf16=w_bf16, kv_bf16=kv_bf16)
    orc = oc.PagedDecoder(params, oc.cfg(SMALL["maxT"], SMALL["V"], L, NH, C), B, P, SMALL["maxT"], page_seed=3,
                          kv_bf16=kv_bf16, w_bf16=w_bf16)
    rng = np.random.default_rng(5)
    # the float64 decoder's own cache: what its kv_rows say the pool stores
    cache = [[(np.zeros((0, C)), np.zeros((0, C))) for _ in range(B)] for _ in range(L)]
    for b, n in enumerate(start):  # a prefix both sides share
        for l in range(L):
            k = rng.uniform(-1, 1, (n, C)).astype(np.float32)
            v = rng.uniform(-1, 1, (n, C)).astype(np.float32)
            if kv_bf16:
                k, v = round_bf16(k), round_bf16(v)
            orc.set_kv(l, b, k, v)
            cache[l][b] = (k.astype(np.float64), v.astype(np.float64))
    pos = np.array(start)
    worst_kv = worst_out = 0.0
    for _ in range(steps):
        tok = rng.integers(0, SMALL["V"], B).astype(np.int32)
        xs = np.zeros((L + 1, B, C), np.float32)
        xs[0] = ref.embed(tok, pos)
        for l in range(L):
            k, v = ref.kv_rows(xs[l], l)
            for b in range(B):
                cache[l][b] = (np.vstack([cache[l][b][0], k[b]]), np.vstack([cache[l][b][1], v[b]]))
            xs[l + 1] = ref.layer_out(xs[l], l, [cache[l][b][0] for b in range(B)],
                                      [cache[l][b][1] for b in range(B)], pos + 1).astype(np.float32)
        _, _, o_out = orc.step_forced(tok, xs)
        for l in range(L):
            ke, ve = ref.kv_rows_exact(xs[l], l)
            okv = [orc.get_kv(l, b, int(pos[b]) + 1) for b in range(B)]
            for b in range(B):
                for got, want in ((okv[b][0][-1], ke[b]), (okv[b][1][-1], ve[b])):
                    d = np.abs(got - want)
                    if kv_bf16:
                        d = np.maximum(d - ref64.half_ulp_bf16(want), 0.0)
                    worst_kv = max(worst_kv, float(d.max() / np.abs(want).max()))
            out = ref.layer_out(xs[l], l, [kv[0] for kv in okv], [kv[1] for kv in okv], pos + 1)
            worst_out = max(worst_out, float(np.abs(out - o_out[l]).max() / np.abs(o_out[l]).max()))
        pos = pos + 1
    orc.close()
    print(f"w_bf16={w_bf16} kv_bf16={kv_bf16}: worst K/V row ratio {worst_kv:.2e}, worst layer ratio {worst_out:.2e}")
    assert worst_kv <= rtol, worst_kv
    assert worst_out <= rtol, worst_out


def test_ragged_positions_of_every_case():
    """the position mix the GPU cases assert, for every (B, P) they use"""
    F = 96
    for B, P in [(64, 16), (33, 8), (5, 64), (17, 32), (17, 8), (64, 64), (33, 32), (8, 16), (5, 16), (21, 8),
                 (70, 16), (20, 32), (1, 16), (40, 8), (200, 8), (96, 8), (4, 16)]:
        pos = ref64.ragged_positions(B, P, F)
        assert pos.min() >= 0 and pos.max() <= F
        for want in [0, P - 1, P, F - 3, F][:B]:
            assert want in pos
        ref64.check_position_mix(pos, P)
    with pytest.raises(AssertionError):
        ref64.check_position_mix(np.full(16, 40), 8)


# ---------------------------------------------------------------- checker self-test
class Scene:
    """three sequences of the C=128 model after two decode steps at ragged
    positions: `before` (random rows, 24 per sequence), the clean `after`
    built from the float64 reference, and the reference rows"""
    F, P, N = 24, 8, 2
    pos = np.array([3, 7, 14])

    def __init__(self, params, kv_bf16):
        self.kv_bf16 = kv_bf16
        self.ref = ref64.Ref64(SMALL, params, kv_bf16=kv_bf16)
        rng = np.random.default_rng(9)
        B = len(self.pos)
        st = (lambda a: round_bf16(a)) if kv_bf16 else (lambda a: a)
        self.before = [[tuple(st(rng.uniform(-1, 1, (self.F, C)).astype(np.float32)) for _ in "KV")
                        for _ in range(B)] for _ in range(L)]
        self.tok = rng.integers(0, SMALL["V"], (self.N, B))
        self.x = rng.normal(0, 0.1, (self.N, L, B, C)).astype(np.float32)  # layer inputs (layer 0: the embedding)
        for s in range(self.N):
            self.x[s, 0] = self.ref.embed(self.tok[s], self.pos + s)
        self.rows = [[[None] * B for _ in range(L)] for _ in "KV"]  # [K|V][l][b] -> (N, C) float64, unrounded
        for l in range(L):
            kv = [self.ref.kv_rows_exact(self.x[s, l], l) for s in range(self.N)]
            for b in range(B):
                for wi in range(2):
                    self.rows[wi][l][b] = np.stack([kv[s][wi][b] for s in range(self.N)])
        self.refs = [[(self.rows[0][l][b], self.rows[1][l][b]) for b in range(B)] for l in range(L)]
        self.after = copy.deepcopy(self.before)
        for l in range(L):
            for b in range(B):
                for wi in range(2):
                    self.after[l][b][wi][self.pos[b]:self.pos[b] + self.N] = self.stored(self.rows[wi][l][b])

    def stored(self, rows):
        r = np.asarray(rows, np.float64).astype(np.float32)
        return round_bf16(r) if self.kv_bf16 else r

    def faulty(self):
        return copy.deepcopy(self.after)

    def check(self, after):
        return ref64.check_kv(self.before, after, self.pos, [self.N] * len(self.pos), ref=self.refs,
                              rtol=FP32_LAYER_RTOL, kv_bf16=self.kv_bf16)


@pytest.fixture(scope="module", params=[False, True], ids=["f32_pool", "bf16_pool"])
def scene(request, params):
    return Scene(params, request.param)


def _fails(scene, after):
    with pytest.raises(ref64.KVMismatch) as e:
        scene.check(after)
    return e.value.faults


def _where(faults):
    return {f[:5] for f in faults}


def test_checker_passes_clean(scene):
    worst = scene.check(scene.after)
    assert worst <= 1e-7  # the fp32 rounding of the reference itself


@pytest.mark.parametrize("shift", [1, -1])
def test_checker_row_at_neighbouring_slot(scene, shift):
    """layer 1, sequence 1: its last appended row lands one slot off"""
    l, b = 1, 1
    t = scene.pos[b] + scene.N - 1
    a = scene.faulty()
    for wi in range(2):
        a[l][b][wi][t + shift] = scene.after[l][b][wi][t]
        a[l][b][wi][t] = scene.before[l][b][wi][t]
    faults = _fails(scene, a)
    assert all(f[:2] == (l, b) for f in faults)
    where = _where(faults)
    for h in range(NH):
        for w in "KV":
            assert (l, b, t, h, w) in where          # the expected row is not there
            assert (l, b, t + shift, h, w) in where  # and its neighbour was touched
    kinds = {p: {f[5] for f in faults if f[2] == p} for p in (t, t + shift)}
    assert kinds[t] == {"unwritten", "value"}  # still the old row, which is not the reference either
    assert kinds[t + shift] == ({"stray"} if shift > 0 else {"value"})  # t - 1 is inside the interval


def test_checker_row_in_next_sequences_page(scene):
    """sequence 0's row of layer 0 goes through sequence 1's block table"""
    l, b = 0, 0
    t = scene.pos[b]
    a = scene.faulty()
    for wi in range(2):
        a[l][b + 1][wi][t] = scene.after[l][b][wi][t]
        a[l][b][wi][t] = scene.before[l][b][wi][t]
    faults = _fails(scene, a)
    where = _where(faults)
    assert {f[:2] for f in faults} == {(l, b), (l, b + 1)}
    for h in range(NH):
        for w in "KV":
            assert (l, b, t, h, w) in where
            assert (l, b + 1, t, h, w) in where
    assert {f[5] for f in faults if f[1] == b} == {"unwritten", "value"}
    assert {f[5] for f in faults if f[1] == b + 1} == {"stray"}  # position 3 is before sequence 1's interval


def test_checker_k_and_v_swapped_for_one_head(scene):
    l, b, h = 1, 2, 1
    t = scene.pos[b]
    a = scene.faulty()
    sl = slice(h * 64, (h + 1) * 64)
    a[l][b][0][t, sl], a[l][b][1][t, sl] = scene.after[l][b][1][t, sl], scene.after[l][b][0][t, sl]
    faults = _fails(scene, a)
    assert _where(faults) == {(l, b, t, h, "K"), (l, b, t, h, "V")}
    assert {f[5] for f in faults} == {"value"}


def test_checker_half_rows_swapped(scene):
    """the two 32-dim halves of one head of one V row"""
    l, b, h = 0, 1, 0
    t = scene.pos[b] + 1
    a = scene.faulty()
    row = scene.after[l][b][1][t, h * 64:(h + 1) * 64]
    a[l][b][1][t, h * 64:(h + 1) * 64] = np.concatenate([row[32:], row[:32]])
    faults = _fails(scene, a)
    assert _where(faults) == {(l, b, t, h, "V")}


def test_checker_row_from_neighbours_position(scene):
    """layer 0: sequence 1's row computed with sequence 2's wpe row"""
    l, b = 0, 1
    a = scene.faulty()
    x = scene.ref.embed(scene.tok[0, b], scene.pos[b + 1])
    k, v = scene.ref.kv_rows_exact(x, l)
    a[l][b][0][scene.pos[b]] = scene.stored(k)
    a[l][b][1][scene.pos[b]] = scene.stored(v)
    faults = _fails(scene, a)
    assert {f[:3] for f in faults} == {(l, b, scene.pos[b])}
    assert {f[4] for f in faults} == {"K", "V"} and {f[5] for f in faults} == {"value"}


def test_checker_bf16_element_truncated(params):
    """one element of a bf16 pool stored by truncation, not nearest-even"""
    scene = Scene(params, True)
    l, b, wi = 1, 0, 0
    t = scene.pos[b]
    r32 = scene.rows[wi][l][b][0].astype(np.float32)
    trunc = from_bf16_bits((r32.view(np.uint32) >> 16).astype(np.uint16))
    excess = np.abs(trunc.astype(np.float64) - scene.rows[wi][l][b][0]) - ref64.half_ulp_bf16(scene.rows[wi][l][b][0])
    i = int(np.argmax(excess))  # the element truncation moves furthest past half an ulp
    assert trunc[i] != round_bf16(r32)[i]
    a = scene.faulty()
    a[l][b][wi][t, i] = trunc[i]
    faults = _fails(scene, a)
    assert _where(faults) == {(l, b, t, i // 64, "K")}


def test_checker_stray_store_before_position(scene):
    l, b, h = 1, 2, 1
    a = scene.faulty()
    a[l][b][1][scene.pos[b] - 4, h * 64 + 5] += np.float32(0.25)
    faults = _fails(scene, a)
    assert [f[:6] for f in faults] == [(l, b, scene.pos[b] - 4, h, "V", "stray")]


def test_checker_expected_row_unwritten(scene):
    l, b = 0, 2
    t = scene.pos[b] + 1
    a = scene.faulty()
    a[l][b][0][t] = scene.before[l][b][0][t]
    faults = _fails(scene, a)
    assert _where(faults) == {(l, b, t, h, "K") for h in range(NH)}
    assert {f[5] for f in faults} == {"unwritten", "value"} and faults[0][5] == "unwritten"


def test_checker_message_names_the_place(scene):
    a = scene.faulty()
    a[1][2][1][0, 70] = 9.0
    with pytest.raises(ref64.KVMismatch, match=r"stray: layer 1 sequence 2 position 0 head 1 V"):
        scene.check(a)
