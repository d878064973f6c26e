"""hpa_paged_attention_verify_packed (bf16 / fp8 pools, chain and tree forms)
against the float64 reference of tests/attn_ref64.py on the values the pool
holds, under the project's BAR.  Batches, poisoned pools and case builders are
those of tests/test_gpu_attention_verify.py and _verify_tree.py; the tree cases'
K and V are rounded to the pool's dtype before the reference is taken."""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
import test_gpu_attention_verify as vc
import test_gpu_attention_verify_tree as vt
from test_attn_ref64 import BAR

pytestmark = pytest.mark.gpu

POOLS = [(ar.HPA_BF16, P) for P in (8, 16, 32, 64)] + [(ar.HPA_FP8, P) for P in (16, 32, 64)]
SHAPES = ("star", "binary", "two_chains", "chain")  # chain: masks that must give the chain form's bits
_F, _I, _U8 = vc._F, vc._I, vt._U8
C = ar.C


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    for key in [k for k in vt._cases if isinstance(k, tuple)]:  # test_tree_against_float64's entries
        del vt._cases[key]


def _packed(hip, s, B, T, anc=None, pool=None):
    """one launch into s's 0xFF-filled output; returns (rc, raw bits)"""
    L = hip.lib()
    hip.check(L.hpa_memset_async(s.d_out.ptr, 0xFF, s.d_out.nbytes))
    c = ctypes.cast
    pool = s.pool.s if pool is None else pool
    rc = L.hpa_paged_attention_verify_packed(c(s.d_q.ptr, _F), ctypes.addressof(pool), 0, c(s.d_bt.ptr, _I),
                                             s.maxp, c(s.d_start.ptr, _I), c(s.d_row0.ptr, _I), c(s.d_len.ptr, _I),
                                             c(anc.ptr, _U8) if anc is not None else None, B, T, c(s.d_out.ptr, _F))
    hip.check(L.hpa_synchronize())
    return rc, s.d_out.download(s.Rp * C).view(np.uint32).copy()


def _check(hip, tag, s, cs, lens, live, anc=None, chain_bits_too=False):
    """at 0 / 4 / 8 waves: every live output finite and within the bar, a second
    launch bit for bit, the len = 0 rows and the frag padding keep their fill;
    chain_bits_too: the chain form on the same inputs gives the same bits"""
    L = hip.lib()
    B, T, R = len(lens), int(lens.max()), len(live)
    kinds = np.array(cs.kind)[live]
    try:
        for waves in (0, 4, 8):
            hip.check(L.hpa_set_attention_waves(waves))
            rc, bits = _packed(hip, s, B, T, anc)
            assert rc == 0
            got = hip.from_frag(bits.view(np.float32), s.Rp, C)
            r = cs.ratios(got[:R])[live]
            print(f"{tag} waves={waves} worst={r.max():.3f} "
                  + " ".join(f"{k}={float(r[kinds == k].max()):.3f}" for k in sorted(set(kinds.ravel()))))
            assert np.isfinite(got[:R][live]).all()
            assert r.max() <= BAR, (tag, waves, np.argwhere(r == r.max())[0], r.max())
            assert (got[:R][~live].view(np.uint32) == 0xFFFFFFFF).all(), "a len = 0 sequence's row was written"
            assert (got[R:].view(np.uint32) == 0xFFFFFFFF).all(), "the frag padding was written"
            for again in [anc] + [None] * chain_bits_too:
                rc2, bits2 = _packed(hip, s, B, T, again)
                assert rc2 == 0 and np.array_equal(bits, bits2), (tag, waves, "chain form" if again is not anc else "twice")
    finally:
        hip.check(L.hpa_set_attention_waves(0))


@pytest.mark.parametrize("dtype,P", POOLS)
def test_chain_against_float64(hip, dtype, P):
    """the five sequences of the fp32 verify test and its edge batch (positions
    60..67 across the tile edge, a len = 0 sequence, 4 rows after it).

    Measured worst ratios per kind on the MI355X (the VERIFYPACKED lines; the
    same for every page size and wave count), against the bar of 40.8: bf16
    pair 2.156, uniform 0.440, hot 0.020, edge batch 0.595; fp8 pair 0.994,
    hot 0.656, uniform 0.559, edge batch 0.190"""
    for name, starts, lens in (("main", vc.STARTS, vc.LENS), ("edge", vc.EDGE_STARTS, vc.EDGE_LENS)):
        s = vc._Set(hip, starts, lens, P, dtype)
        live = np.repeat(s.lens > 0, np.maximum(s.lens, 1))
        _check(hip, f"VERIFYPACKED {name} dtype={dtype} P={P}", s, s.cs, s.lens, live)


def _rounded(shape, dtype):
    """the fp32 tree test's cases with each sequence's K and V rounded in place
    to the pool's dtype as the constructor stores them in seqs, which is before
    it aims a query at them or takes a reference or a leak from them"""
    class Seqs(list):
        def append(self, kv):
            # the node V rows (up to 161 in size) stay inside the range (448 x the smaller fp8 scale = 224) and keep
            # their distance: relative rounding error <= 2^-8 (bf16, 8 significant bits) / 2^-4 (e4m3, 4)
            rel = 2.0 ** -8 if dtype == ar.HPA_BF16 else 2.0 ** -4
            for a, scale in zip(kv, ar._scales(dtype)):
                r = ar.round_pool(a, dtype, scale)
                assert np.abs(a).max() < 448 * 0.5 and (np.abs(r - a) <= rel * np.abs(a) + 2.0 ** -9).all()
                a[:] = r
            super().append(kv)

    class Cases(vt._TreeCases):
        seqs = property(lambda self: self._seqs, lambda self, _: setattr(self, "_seqs", Seqs()))
    return Cases(shape)


@pytest.mark.parametrize("dtype,P", POOLS)
@pytest.mark.parametrize("shape", SHAPES)
def test_tree_against_float64(hip, shape, dtype, P):
    """the six sequences of the fp32 tree test: a leak of the aimed-at hidden
    key would move the output by more than 100 units (asserted in float64
    first); chain masks give the chain form's bits.

    Measured worst ratios per kind on the MI355X (the TREEPACKED lines, over
    every shape, page size and wave count), against the bar of 40.8: bf16
    hot_hidden 1.054, uniform 0.603, hot_parent 0.048, hot_own 0.034; fp8
    uniform 0.867, hot_hidden 0.483, hot_key0 0.058, hot_own 0.053"""
    key = (shape, dtype)  # vt._Set looks its cases up in vt._cases; the fp32 test's keys there are plain shapes
    if key not in vt._cases:
        vt._cases[key] = _rounded(shape, dtype)
    s = vt._Set(hip, key, P, dtype)
    cs = s.cs
    leak = cs.leak[~np.isnan(cs.leak)]
    assert leak.size >= 12 and leak.min() > 100.0, (leak.size, leak.min())
    if shape == "chain":
        assert cs.anc[cs.live].tolist() == [(2 << (i - cs.row0[b])) - 1 for i, b in enumerate(cs.seq) if cs.live[i]]
    _check(hip, f"TREEPACKED {shape} dtype={dtype} P={P}", s, cs, cs.lens, cs.live, s.d_anc, shape == "chain")


def test_refusals(hip):
    """an fp32 pool, T = 0, T = 9, an fp8 pool of page size 8: nonzero and the output keeps its fill"""
    s, f32, f8 = (vc._Set(hip, vc.EDGE_STARTS, vc.EDGE_LENS, 16, dt) for dt in (ar.HPA_BF16, ar.HPA_F32, ar.HPA_FP8))
    p8 = type(f8.pool.s)()
    ctypes.memmove(ctypes.addressof(p8), ctypes.addressof(f8.pool.s), ctypes.sizeof(p8))
    p8.page_size = 8  # refused on the struct's fields, before anything is launched
    for what, T, pool in ((s, 0, None), (s, 9, None), (f32, 8, None), (f8, 8, p8)):
        rc, bits = _packed(hip, what, len(s.lens), T, pool=pool)
        assert rc != 0 and (bits == 0xFFFFFFFF).all(), (T, pool)
