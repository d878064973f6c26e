"""The greedy pick, kernel by kernel, where every logit is negative and where
maxima tie exactly (tests/pick_inputs.py: `shifted` and `ties` (a), (b), (c)).

Every producer of (max, argmax) row partials -- the looped fp32 epilogue, the
two resident logits kernels and their in-launch pick, stream-K, the bf16
looped and A-resident kernels, the SCORE epilogue, the row_seq LOGITS form --
and both reducers (hpa_argmax_final, hpa_score_final) run on both
constructions.  Descriptors are built as test_gpu_fused.py::_run builds them.

Per case:
  * stored logits within gemm_bounds' bound of the float64 product (shifted),
    or bit-equal on the expected columns and below them elsewhere (ties)
  * check_partials: every partial's column < N (or the empty marker), its
    value the maximum of its live columns bit for bit, padded rows not finite
  * check_pick: 0 <= id < N, id == the first argmax of the path's own logits;
    on ties the ids are min(E) / min(O) row by row
  * out rows >= M and 64 guard words after out, part_out and next untouched

Shapes: K = 768, N = 9601 (601 column tiles, more than twice the CU count:
resident workgroups and bf16 rounds own several tiles; one live column in the
last tile); K = 1600, N = 2001 on stream-K (126 tiles, 63 super-tiles, one
live column in the last); one N = 50257 case on the resident kernel.

Measured (MI355X), worst |gpu - f64| / bound on `shifted` (the file runs in 3.2 s):
  looped fp32 0.045 | resident 12 0.045 (N = 50257: 0.049) | resident 16 0.027 | stream-K 0.022
  bf16 looped 0.58 | bf16 A-resident 0.67 | SCORE |logprob - f64| / kernel_bound: fp32 0.076, bf16 0.080
No path refused a listed combination; no defect found.
"""
import ctypes
import functools

import numpy as np
import pytest

import pick_inputs as pi
import score_ref64 as sr
from test_gpu_fused import _stats_tiles
from test_gpu_score_kernel import _check as score_check

pytestmark = pytest.mark.gpu

KINDS = ["shifted", "ties_a", "ties_b", "ties_c"]
SENT = np.uint32(0x7FC0DEAD)  # a NaN no kernel computes
GUARD = 64
RATIOS = {}  # path -> worst |gpu - f64| / bound on `shifted`


@functools.lru_cache(maxsize=8)
def _host(kind, K, N, bf16, rows):
    """the construction at `rows` rows (a launch of M rows takes the first M:
    the rows are independent and the ties' parity starts at row 0)"""
    if kind == "shifted":
        inp = pi.shifted(rows, K, N, seed=K + N, w_bf16=bf16)
        pi.check_shifted_inputs(inp)
    else:
        E, O = pi.tie_sets(N)[kind[-1]]
        inp = pi.ties(rows, K, N, E, O)
        pi.check_ties_inputs(inp)
    return inp


_DEV_W = {}


def _dev_w(hip, kind, K, N, bf16, W):
    """the packed weights on the device, kept across the cases of a construction"""
    key = (kind, K, N, bf16)
    if key not in _DEV_W:
        if len(_DEV_W) >= 4:
            _DEV_W.pop(next(iter(_DEV_W)))
        L = hip.lib()
        src = hip.DeviceBuffer.from_array(W)
        if bf16:
            dst = hip.DeviceBuffer(L.hpa_frag_bf16_elems(N, K) * 2)
            hip.check(L.hpa_pack_frag_bf16(src.ptr, N, K, K, dst.ptr), "pack bf16")
        else:
            dst = hip.DeviceBuffer(L.hpa_frag_elems(N, K) * 4)
            hip.check(L.hpa_pack_frag(src.ptr, N, K, K, dst.ptr), "pack")
        hip.check(L.hpa_synchronize())
        _DEV_W[key] = dst
    return _DEV_W[key]


def _guarded(hip, words):
    """`words` 4-byte words plus the guard, all holding the sentinel"""
    return hip.DeviceBuffer.from_array(np.full(words + GUARD, SENT, np.uint32))


def _untouched(buf, lo, hi=None):
    w = buf.download(buf.nbytes // 4, np.uint32)
    assert np.all(w[lo:hi] == SENT), np.flatnonzero(w[lo:hi] != SENT)[:8] + lo


class _Launch:
    """one LOGITS (or SCORE) launch of the first M rows of a construction"""

    def __init__(self, hip, kind, K, N, M, bf16=False, variant=1, waves=0, rb=0, ct=0, sk=False, rows=256,
                 out_rows=None, row_seq=None):
        self.hip, self.L = hip, hip.lib()
        self.inp = inp = _host(kind, K, N, bf16, rows)
        self.kind, self.K, self.N, self.M, self.Mp = kind, K, N, M, (M + 15) // 16 * 16
        self.ntiles = (N + 15) // 16
        self.keep = []
        x = inp["x"][:M]
        g = self.g = hip.HpaFusedGemm()
        g.x, g.M, g.K, g.N = self._dev(hip.to_frag(x)), M, K, N
        g.ln_stats, g.ln_ntiles = self._dev(_stats_tiles(x, self.Mp)), K // 16
        g.ln_w, g.ln_b = self._dev(inp["lw"]), self._dev(inp["lb"])
        g.w = _dev_w(hip, kind, K, N, bf16, inp["W"]).ptr
        g.w_dtype = hip.HPA_BF16 if bf16 else hip.HPA_F32
        g.waves, g.row_blocks, g.col_tiles, g.variant = waves, rb, ct, variant
        self.out_rows = self.Mp if out_rows is None else out_rows
        self.row_seq = row_seq
        if row_seq is not None:
            g.row_seq = self._dev(np.asarray(row_seq, np.int32))
        self.cnt = None
        if sk:  # stream-K workspace: zeroed once; every launch leaves the counters zero
            nf, nc = ctypes.c_size_t(), ctypes.c_size_t()
            hip.check(self.L.hpa_gemm_sk_workspace(N, ctypes.byref(nf), ctypes.byref(nc)), "sk workspace")
            slab = hip.DeviceBuffer(nf.value * 4)
            self.cnt = hip.DeviceBuffer.from_array(np.zeros(nc.value, np.int32))
            self.keep += [slab]
            g.sk_slab, g.sk_count = slab.ptr, self.cnt.ptr

    def _dev(self, a):
        b = self.hip.DeviceBuffer.from_array(np.ascontiguousarray(a))
        self.keep.append(b)
        return b.ptr

    def logits(self):
        """runs HPA_FEPI_LOGITS; returns (own logits (M, N) by GEMM row, partials (npart, Mp, 2))"""
        hip, g, M, N = self.hip, self.g, self.M, self.N
        self.out = _guarded(hip, self.out_rows * N)
        self.part = _guarded(hip, self.ntiles * self.Mp * 2)
        g.epilogue, g.out, g.part_out = hip.HPA_FEPI_LOGITS, self.out.ptr, self.part.ptr
        self.npart = self.L.hpa_logits_partials(ctypes.byref(g))
        assert 0 < self.npart <= self.ntiles
        hip.check(self.L.hpa_gemm_fused(ctypes.byref(g)), "gemm_fused LOGITS")
        hip.check(self.L.hpa_synchronize())
        return self.read()

    def read(self):
        M, N = self.M, self.N
        full = self.out.download((self.out_rows, N))
        dest = np.arange(M) if self.row_seq is None else np.asarray(self.row_seq)
        # every out row no GEMM row names, and the guard after out and after the partials
        other = np.ones(self.out_rows, bool)
        other[dest] = False
        assert np.all(full[other].view(np.uint32) == SENT)
        _untouched(self.out, self.out_rows * N)
        _untouched(self.part, self.npart * self.Mp * 2)
        part = self.part.download((self.npart, self.Mp, 2))
        if self.cnt is not None:
            assert not self.cnt.download(self.cnt.nbytes // 4, np.int32).any()
        return full[dest], part

    def final(self, active=None, tokens=False, pos=False):
        """hpa_argmax_final on the launch's partials: (next, tokens, pos) after it,
        each started from a sentinel (-7, -7, 100 + row) and followed by a guard"""
        hip, M = self.hip, self.M
        nxt = hip.DeviceBuffer.from_array(np.full(M + GUARD, -7, np.int32))
        tok = hip.DeviceBuffer.from_array(np.full(M + GUARD, -7, np.int32))
        ps = hip.DeviceBuffer.from_array(100 + np.arange(M + GUARD, dtype=np.int32))
        act = None if active is None else hip.DeviceBuffer.from_array(np.asarray(active, np.int32))
        hip.check(self.L.hpa_argmax_final(self.part.ptr, self.npart, self.Mp, M, nxt.ptr, tok.ptr if tokens else None,
                                          ps.ptr if pos else None, act.ptr if act is not None else None), "argmax_final")
        hip.check(self.L.hpa_synchronize())
        n, t, p = (b.download(M + GUARD, np.int32) for b in (nxt, tok, ps))
        assert np.all(n[M:] == -7) and np.all(t[M:] == -7) and np.array_equal(p[M:], 100 + np.arange(M, M + GUARD))
        return n[:M], t[:M], p[:M]


def _owner(layout, ntiles, npart):
    if layout == "tiles":
        assert npart == ntiles
        return None
    return pi.tile_owner_strided(ntiles, npart) if layout == "strided" else pi.tile_owner_runs(ntiles, npart)


def _assert_case(c, x, part, ids, path, layout="tiles"):
    """the per-case assertions on a path's own logits x, partials and ids"""
    inp, M, N = c.inp, c.M, c.N
    if c.kind == "shifted":
        ratio = float((np.abs(x - inp["acc"][:M]) / inp["bound"][:M]).max())
        RATIOS[path] = max(RATIOS.get(path, 0.0), ratio)
        print(f"{path}: shifted worst |gpu - f64| / bound {ratio:.3f} (worst per path so far {RATIOS[path]:.3f})")
        assert ratio <= 1.0, ratio
        assert x.max() <= -1.0
    else:
        pi.check_tied_logits(x, inp)
    pi.check_partials(part, x, N, M, _owner(layout, c.ntiles, part.shape[0]))
    pi.check_pick(ids, x, N)
    if c.kind != "shifted":
        assert np.array_equal(ids, inp["want"][:M])


LOOPED = [(64, 4, 4, 1, 1), (64, 8, 1, 1, 1), (64, 16, 2, 1, 1), (64, 4, 4, 2, 1), (64, 4, 4, 4, 1), (64, 8, 4, 2, 1),
          (37, 4, 4, 1, 1), (37, 8, 1, 1, 1), (37, 16, 2, 1, 1), (37, 4, 4, 2, 1), (37, 4, 4, 4, 1), (37, 8, 4, 2, 1),
          (130, 0, 0, 0, 0)]


@pytest.mark.parametrize("M,waves,rb,ct,variant", LOOPED)
@pytest.mark.parametrize("kind", KINDS)
def test_looped_fp32(hip, kind, M, waves, rb, ct, variant):
    """the looped kernel's Epi: one, two and four column tiles per workgroup,
    1 / 2 / 4 row blocks, 37 rows (11 padded) and 130 rows by shape"""
    c = _Launch(hip, kind, 768, 9601, M, variant=variant, waves=waves, rb=rb, ct=ct)
    x, part = c.logits()
    _assert_case(c, x, part, c.final()[0], "looped fp32")


@pytest.mark.parametrize("form,layout", [(12, "runs"), (16, "strided")])
@pytest.mark.parametrize("M", [64, 37, 16, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_resident(hip, kind, form, layout, M):
    """variant 4, both forms: one running partial per row per workgroup (256
    workgroups own 2 or 3 of the 601 tiles each -- a contiguous run in the
    ring form, a stride of 256 in the 16-wave form), reduced by
    hpa_argmax_final, then by the in-launch pick on three launches back to
    back (counter left 0, pos += 1 per launch)"""
    c = _Launch(hip, kind, 768, 9601, M, variant=4, waves=form)
    x, part = c.logits()
    assert part.shape[0] <= 256 < c.ntiles  # one partial per workgroup, several tiles each
    path = f"resident form {form}"
    _assert_case(c, x, part, c.final()[0], path, layout)
    _in_launch_pick(c, x, part, path, layout)


def _in_launch_pick(c, x, part, path, layout):
    hip, g, M = c.hip, c.g, c.M
    nxt = hip.DeviceBuffer.from_array(np.full(M + GUARD, -7, np.int32))
    tok = hip.DeviceBuffer.from_array(np.full(M + GUARD, -7, np.int32))
    pos = hip.DeviceBuffer.from_array(100 + np.arange(M + GUARD, dtype=np.int32))
    cnt = hip.DeviceBuffer.from_array(np.zeros(1 + GUARD, np.int32))
    g.pick_next, g.pick_tokens, g.pick_pos, g.pick_count = nxt.ptr, tok.ptr, pos.ptr, cnt.ptr
    for it in range(3):
        hip.check(c.L.hpa_gemm_fused(ctypes.byref(g)), "gemm_fused pick")
        hip.check(c.L.hpa_synchronize())
        x2, part2 = c.read()
        assert np.array_equal(x2.view(np.uint32), x.view(np.uint32))
        assert np.array_equal(part2.view(np.uint32), part.view(np.uint32))
        n, t, p = (b.download(M + GUARD, np.int32) for b in (nxt, tok, pos))
        _assert_case(c, x, part, n[:M], path + " in-launch pick", layout)
        assert np.array_equal(t[:M], n[:M])
        assert np.array_equal(p[:M], 100 + np.arange(M) + it + 1)
        assert np.all(n[M:] == -7) and np.all(t[M:] == -7) and np.array_equal(p[M:], 100 + np.arange(M, M + GUARD))
        assert not cnt.download(1 + GUARD, np.int32).any()
    g.pick_next = g.pick_tokens = g.pick_pos = g.pick_count = None


@pytest.mark.parametrize("kind", ["shifted", "ties_a"])
def test_resident_full_vocabulary(hip, kind):
    """N = 50257 (3142 tiles: 12 or 13 per workgroup), the engine's form at 64 rows"""
    c = _Launch(hip, kind, 768, 50257, 64, variant=4, waves=12, rows=64)
    x, part = c.logits()
    _assert_case(c, x, part, c.final()[0], "resident form 12, N = 50257", "runs")
    _in_launch_pick(c, x, part, "resident form 12, N = 50257", "runs")


@pytest.mark.parametrize("variant", [6, 4])
@pytest.mark.parametrize("M", [64, 37, 16, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_stream_k(hip, kind, variant, M):
    """stream-K (variant 6, and variant 4 given a stream-K workspace: GPT-2
    XL's logits path), K = 1600 with the LayerNorm applied on load, N = 2001:
    63 super-tiles over the CUs, so tiles are split between workgroups and
    summed by the last to arrive; the counters are zero afterwards"""
    K, N = 1600, 2001
    assert hip.lib().hpa_logits_kernel(M, N, K) == 6
    c = _Launch(hip, kind, K, N, M, variant=variant, waves=8, sk=True)
    x, part = c.logits()
    _assert_case(c, x, part, c.final()[0], "stream-K")
    if variant == 4:  # the engine's launch: pick_* given, picked by hpa_argmax_final after the GEMM
        _in_launch_pick(c, x, part, "stream-K", "tiles")


@pytest.mark.parametrize("M,waves,rb,ct,variant", [(64, 4, 4, 2, 1), (37, 4, 4, 2, 1), (64, 8, 2, 1, 1), (37, 8, 2, 1, 1),
                                                   # A-resident: ct = rounds (4, 8, 0 = automatic)
                                                   (64, 8, 4, 4, 5), (50, 8, 4, 4, 5), (256, 8, 4, 4, 5),
                                                   (64, 8, 2, 8, 5), (50, 8, 2, 8, 5), (256, 8, 2, 8, 5),
                                                   (64, 8, 4, 0, 5), (50, 8, 4, 0, 5), (256, 8, 4, 0, 5)])
@pytest.mark.parametrize("kind", KINDS)
def test_bf16(hip, kind, M, waves, rb, ct, variant):
    """bf16 weights (config 5's logits path): the looped kernel and the
    A-resident one, whose waves walk waves * rounds column tiles"""
    c = _Launch(hip, kind, 768, 9601, M, bf16=True, variant=variant, waves=waves, rb=rb, ct=ct)
    x, part = c.logits()
    _assert_case(c, x, part, c.final()[0], "bf16 looped" if variant == 1 else "bf16 A-resident")


@pytest.mark.parametrize("kind", ["shifted", "ties_a"])
@pytest.mark.parametrize("bf16,variant,waves,rb,ct", [(False, 1, 4, 4, 2), (False, 1, 8, 1, 1), (True, 1, 4, 4, 2),
                                                      (True, 5, 8, 4, 0)])
def test_row_seq_logits(hip, kind, bf16, variant, waves, rb, ct):
    """row_seq LOGITS (gpt2_forward's per-position logits written in place):
    GEMM row m lands in out row row_seq[m], a permutation into 45 rows; the
    8 rows no GEMM row names keep the sentinel; partials stay by GEMM row"""
    M, R = 37, 45
    seq = np.random.default_rng(9).permutation(R)[:M].astype(np.int32)
    assert not np.array_equal(seq, np.arange(M)) and len(set(seq.tolist())) == M and seq.max() >= M
    c = _Launch(hip, kind, 768, 9601, M, bf16=bf16, variant=variant, waves=waves, rb=rb, ct=ct, out_rows=R,
                row_seq=seq)
    x, part = c.logits()
    _assert_case(c, x, part, c.final()[0], "row_seq " + ("bf16" if bf16 else "fp32"))


@pytest.mark.parametrize("path", ["looped", "resident12", "resident16"])
@pytest.mark.parametrize("kind", KINDS)
def test_argmax_final_active_mask(hip, kind, path):
    """hpa_argmax_final on the same partials with `active` mixing 1, 0 and -1
    (and 2): inactive rows keep their sentinel next / tokens / pos, active
    rows get next = tokens = the pick and pos += 1 exactly once; tokens and
    pos NULL leave those arrays alone"""
    M = 37
    if path == "looped":
        c = _Launch(hip, kind, 768, 9601, M, variant=1, waves=4, rb=4, ct=2)
    else:
        c = _Launch(hip, kind, 768, 9601, M, variant=4, waves=int(path[-2:]))
    x, _ = c.logits()
    want = sr.first_argmax(x).astype(np.int32)
    active = np.resize(np.array([1, 0, -1, 2, 1, 1, 0], np.int32), M)
    active[M - 1] = 0
    on = active > 0
    before = (np.full(M, -7, np.int32), np.full(M, -7, np.int32), 100 + np.arange(M, dtype=np.int32))
    n, t, p = c.final(active=active, tokens=True, pos=True)
    for b, a in zip(before, (n, t, p)):
        pi.check_untouched(active, b, a)
    pi.check_pick(n[on], x[on], c.N)
    assert np.array_equal(n[on], want[on]) and np.array_equal(t[on], want[on])
    assert np.array_equal(p[on], before[2][on] + 1)
    n2, t2, p2 = c.final(active=active)  # tokens / pos NULL
    assert np.array_equal(n2, n) and np.array_equal(t2, before[1]) and np.array_equal(p2, before[2])
    n3, t3, p3 = c.final(tokens=True, pos=True)  # active NULL: every row
    pi.check_pick(n3, x, c.N)
    assert np.array_equal(t3, n3) and np.array_equal(p3, before[2] + 1)
    off = np.zeros(M, np.int32)
    off[::2] = -1
    n4, t4, p4 = c.final(active=off, tokens=True, pos=True)  # nothing active
    assert np.array_equal(n4, before[0]) and np.array_equal(t4, before[1]) and np.array_equal(p4, before[2])


SCORE_RATIO = [0.0]


@pytest.mark.parametrize("kind", ["shifted", "ties_a", "ties_b"])
@pytest.mark.parametrize("M,bf16,variant,waves,rb,ct", [(37, False, 0, 0, 0, 0), (64, False, 1, 4, 4, 4),
                                                        (64, False, 1, 8, 4, 2), (37, False, 1, 16, 1, 1),
                                                        (37, True, 0, 0, 0, 0), (64, True, 1, 4, 2, 2),
                                                        (37, True, 1, 8, 1, 1), (64, True, 5, 8, 4, 0),
                                                        (50, True, 5, 4, 1, 2)])
def test_score_epilogue(hip, kind, M, bf16, variant, waves, rb, ct):
    """HPA_FEPI_SCORE + hpa_score_final against the path's own LOGITS output,
    held to tests/score_ref64.py as test_gpu_score_kernel.py::_check holds it
    (top id == the first argmax exactly, log-probabilities within
    kernel_bound); the partials' (.x, .w) as the LOGITS partials; targets
    include column N - 1, a tied column and none"""
    K, N = 768, 9601
    c = _Launch(hip, kind, K, N, M, bf16=bf16, variant=variant, waves=waves, rb=rb, ct=ct)
    x, _ = c.logits()
    L, g, Mp = c.L, c.g, c.Mp
    t = np.random.default_rng(M).integers(0, N, M).astype(np.int32)
    tied = 4001 if kind == "shifted" else max(c.inp["E"])
    t[:7] = [0, N - 1, tied, -1, 15, 16, N - 2]
    t[M - 1] = N - 1
    nf = ctypes.c_size_t()
    hip.check(L.hpa_score_workspace(N, Mp, ctypes.byref(nf)), "workspace")
    assert nf.value == c.ntiles * Mp * 4
    sp = _guarded(hip, nf.value)
    g.epilogue, g.out, g.part_out = hip.HPA_FEPI_SCORE, None, None
    g.score_target, g.score_part = c._dev(t), sp.ptr
    hip.check(L.hpa_gemm_fused(ctypes.byref(g)), "SCORE")
    lp, lse, tlp, top = (_guarded(hip, M) for _ in range(4))
    hip.check(L.hpa_score_final(sp.ptr, c.ntiles, Mp, M, lp.ptr, lse.ptr, top.ptr, tlp.ptr), "score_final")
    hip.check(L.hpa_synchronize())
    for b in (lp, lse, tlp, top):
        _untouched(b, M)
    _untouched(sp, nf.value)
    part = sp.download((c.ntiles, Mp, 4))
    assert not np.isnan(part).any()
    pi.check_partials(np.ascontiguousarray(part[..., [0, 3]]), x, N, M)
    tl = part[..., 2]  # the target's logit in its tile, -inf elsewhere
    live = np.flatnonzero(t >= 0)
    assert np.array_equal(tl[t[live] // 16, live].view(np.uint32), x[live, t[live]].view(np.uint32))
    assert np.isinf(tl).sum() == tl.size - len(live)
    lpv, lsev, tlpv, topv = lp.download(M), lse.download(M), tlp.download(M), top.download(M, np.int32)
    score_check(x, t, lpv, lsev, topv, tlpv)
    pi.check_pick(topv, x, N)
    if kind != "shifted":
        assert np.array_equal(topv, c.inp["want"][:M])
    ratio = float((np.abs(lpv.astype(np.float64) - sr.logprob64(x, t)) / sr.kernel_bound(x, t)).max())
    SCORE_RATIO[0] = max(SCORE_RATIO[0], ratio)
    print(f"SCORE {'bf16' if bf16 else 'fp32'} variant {variant}: worst |logprob - f64| / kernel_bound {ratio:.3f} "
          f"(worst so far {SCORE_RATIO[0]:.3f})")
