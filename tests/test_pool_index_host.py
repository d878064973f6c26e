"""The host side of the page-pool addressing, without a GPU: hpa_pool_tile,
hpa_pool_k_index and hpa_pool_v_index on hand-filled HpaKVPool structs (no
allocation; base 0 or a made-up address) against the same formula in Python
integers, on pools of up to 2^31 - 1 pages and 64 layers; the block manager at
a few hundred thousand blocks; and the 32-bit models of tests/pool_marks.py
against the library at the pages tests/test_gpu_pool_large.py uses.

Layout (include/hip_paged_attn.h), in elements of the pool's dtype:

    tile(layer, page, kv, head) = layer layer_elems + page page_elems + (kv NH + head) P hs
    K(slot, d) = tile + ((d // CH) P + slot) CH + d % CH     CH = 4 / 8 / 16 (fp32 / bf16 / fp8)
    V(slot, d) = tile + slot hs + d

Pages checked per pool: 0, the three pages around every mark of pool_marks
(2^31 and 2^32 bytes, 2^31 and 2^32 elements from the layer's base) that lies
inside the layer, and the last page -- in layer 0 and in the last layer.
"""
import ctypes
import itertools

import numpy as np
import pytest

import pagedattn as pa
import pool_marks as pm

HS = 64
BASES = (0, 0x7F12_3456_0000)


def _pool(L, NH, P, num_pages, dtype, base):
    """the fields hpa_pool_create sets, by hand"""
    s = pa.HpaKVPool()
    s.base = base
    s.num_layers, s.num_heads, s.head_size, s.page_size, s.num_pages, s.dtype = L, NH, HS, P, num_pages, dtype
    s.elem_bytes = pm.ELEM_BYTES[dtype]
    s.page_elems = pm.page_elems(NH, P, HS)
    s.layer_elems = num_pages * s.page_elems
    s.bytes = L * s.layer_elems * s.elem_bytes
    s.managed = 0
    s.scales = None
    assert s.bytes == L * num_pages * pm.page_elems(NH, P, HS) * pm.ELEM_BYTES[dtype]  # fits 64 bits
    return s


def _tile(s, layer, page, kv, head):
    return layer * s.layer_elems + page * s.page_elems + (kv * s.num_heads + head) * s.page_size * HS


def _k(s, layer, page, head, slot, d):
    ch = pm.K_CHUNK[s.dtype]
    return _tile(s, layer, page, 0, head) + ((d // ch) * s.page_size + slot) * ch + d % ch


def _v(s, layer, page, head, slot, d):
    return _tile(s, layer, page, 1, head) + slot * HS + d


def _pages(s):
    pb = s.page_elems * s.elem_bytes
    out = {0, s.num_pages - 1}
    for m in pm.marks(s.num_pages * pb, s.elem_bytes):
        out |= {m // pb - 1, m // pb, m // pb + 1}
    return sorted(p for p in out if 0 <= p < s.num_pages)


POOLS = [(L, NH, P, n, dt)
         for (L, n) in ((1, 2 ** 31 - 1), (64, 2 ** 31 - 1), (2, 600_000), (12, 2_200_000), (1, 17))
         for NH in (2, 12, 25)
         for dt, P in ((pm.F32, 8), (pm.F32, 64), (pm.BF16, 8), (pm.BF16, 32), (pm.FP8, 16), (pm.FP8, 64))]


@pytest.mark.parametrize("base", BASES, ids=["base0", "base"])
def test_index_functions_match_python_integers(base):
    lib = pa.lib()
    checked = above = 0
    for L, NH, P, n, dt in POOLS:
        s = _pool(L, NH, P, n, dt, base)
        ref = ctypes.byref(s)
        pages = _pages(s)
        assert pages[0] == 0 and pages[-1] == n - 1
        if n > 2 ** 30:
            assert len(pm.marks(n * s.page_elems * s.elem_bytes, s.elem_bytes)) == len({1, 2, s.elem_bytes, 2 * s.elem_bytes})
        for layer, page in itertools.product(sorted({0, L - 1}), pages):
            for kv, head in ((0, 0), (1, 0), (0, NH - 1), (1, NH - 1)):
                got = lib.hpa_pool_tile(ref, layer, page, kv, head) or 0
                assert got == base + _tile(s, layer, page, kv, head) * s.elem_bytes, (L, NH, P, n, dt, layer, page, kv, head)
            for head, slot, d in ((0, 0, 0), (NH - 1, P - 1, HS - 1), (NH // 2, P // 2 + 1, 37)):
                assert lib.hpa_pool_k_index(ref, layer, page, head, slot, d) == _k(s, layer, page, head, slot, d), \
                    (L, NH, P, n, dt, layer, page, head, slot, d)
                assert lib.hpa_pool_v_index(ref, layer, page, head, slot, d) == _v(s, layer, page, head, slot, d), \
                    (L, NH, P, n, dt, layer, page, head, slot, d)
            checked += 1
            above += page * s.page_elems >= 2 ** 32
    # the last page of the last layer of the largest pool: about 2^56 bytes from the base
    s = _pool(64, 25, 64, 2 ** 31 - 1, pm.F32, base)
    assert _v(s, 63, 2 ** 31 - 2, 24, 63, 63) * 4 + 4 == s.bytes > 2 ** 56
    assert checked > 1000 and above > 200, (checked, above)


def test_k_and_v_indices_tile_a_page_exactly():
    """inside one page past 2^32 elements the K and V indices of every (head,
    slot, d) are a permutation of the page's elements"""
    lib = pa.lib()
    for dt, P in ((pm.F32, 8), (pm.BF16, 8), (pm.FP8, 16)):
        NH = 2
        s = _pool(2, NH, P, 2 ** 24, dt, 0)
        page = 2 ** 32 // s.page_elems + 3
        ref = ctypes.byref(s)
        idx = [fn(ref, 1, page, h, slot, d) for fn in (lib.hpa_pool_k_index, lib.hpa_pool_v_index)
               for h in range(NH) for slot in range(P) for d in range(HS)]
        lo = s.layer_elems + page * s.page_elems
        assert sorted(idx) == list(range(lo, lo + s.page_elems)), (dt, P)


def _big_pool_shapes():
    """(what, dtype, NH, P, layer bytes): every pool of tests/test_gpu_pool_large.py"""
    out = []
    for dt in (pm.F32, pm.BF16, pm.FP8):
        for P in (pm.MIN_PAGE[dt], 64):
            out.append((f"standalone-{dt}-P{P}", dt, 2, P, pm.BIG_LAYER_BYTES[dt]))
    for dt, NH, P in ((pm.F32, 12, 16), (pm.BF16, 12, 8), (pm.FP8, 12, 16), (pm.BF16, 16, 32), (pm.F32, 2, 16)):
        out.append((f"engine-{dt}-NH{NH}-P{P}", dt, NH, P, pm.ENGINE_LAYER_BYTES))
    return out


@pytest.mark.parametrize("need", [40, 700, 2100])
def test_a_32_bit_offset_is_wrong_at_every_page_the_gpu_tests_place_above_a_mark(need):
    """the four 32-bit models of pool_marks.MODELS against hpa_pool_tile on the
    candidate pages of every big pool: equal below the model's mark, different
    at every page that starts at or above it.  So a kernel that formed the
    page offset in any of those types would read or write the wrong page
    there: the chosen pages would expose it."""
    lib = pa.lib()
    for what, dt, NH, P, layer_bytes in _big_pool_shapes():
        if what.startswith("engine") and need > 700:  # a batch of 20 sequences: a few hundred pages at the most
            continue
        eb = pm.ELEM_BYTES[dt]
        pe = pm.page_elems(NH, P)
        n = pm.engine_pages(pe * eb) if what.startswith("engine") else layer_bytes // (pe * eb)
        s = _pool(1, NH, P, n, dt, 0)
        mk = pm.marks(n * pe * eb, eb)
        assert mk and mk[0] == 2 ** 31, what
        cand = pm.candidates(n, pe * eb, mk, need)
        used = cand[:need]
        assert {0, n - 1} <= set(used.tolist())
        for m, (lo, hi) in pm.sides(used, pe * eb, mk).items():
            assert lo >= need // (2 * len(mk) + 2) and hi >= need // (2 * len(mk) + 2), (what, m, lo, hi)
        wrong = {k: 0 for k in pm.MODELS}
        for page in used.tolist():
            true = lib.hpa_pool_tile(ctypes.byref(s), 0, page, 0, 0) or 0
            assert true == page * pe * eb
            for name, (thr, model) in pm.MODELS.items():
                if true >= thr(eb):
                    assert model(page, pe, eb) != true, (what, name, page)
                    wrong[name] += 1
                elif (page + 1) * pe * eb <= thr(eb):
                    assert model(page, pe, eb) == true, (what, name, page)
        for name, (thr, _) in pm.MODELS.items():
            assert (wrong[name] > 0) == (thr(eb) in mk), (what, name, wrong)


def test_block_manager_at_a_few_hundred_thousand_blocks():
    """create_block_manager_ex at the page count of a 4 GiB fp32 layer (C = 768,
    P = 16): first-fit order, the page lists, and reuse of freed low pages"""
    nblocks, per, prompts = 300_000, 3000, 120
    bm = pa.BlockManager(1, prompts, nblocks, 1, per, host_pages=True)
    try:
        assert bm.free_pages() == nblocks
        got = np.empty(nblocks, np.int64)
        k = 0
        for p in range(100):  # 100 prompts x 3000 pages: every page, in order
            for _ in range(per):
                got[k] = bm.request_block(p)
                k += 1
        assert k == nblocks and np.array_equal(got, np.arange(nblocks)) and bm.free_pages() == 0
        for p in (0, 57, 99):
            assert bm.pages(p) == list(range(p * per, (p + 1) * per))
        assert bm.request_block(3) == -1  # a full per-prompt list refuses
        for p in (99, 7, 50):
            bm.free_prompt(p)
        assert bm.free_pages() == 3 * per
        want = list(range(7 * per, 8 * per)) + list(range(50 * per, 50 * per + 10))
        assert [bm.request_block(110) for _ in range(per)] + [bm.request_block(111) for _ in range(10)] == want
        assert bm.pages(110) == want[:per] and bm.pages(111) == want[per:]
        assert bm.pages(8) == list(range(8 * per, 9 * per))  # a neighbour's list untouched
        assert bm.refs(nblocks - 1) == 0 and bm.refs(7 * per) == 1
    finally:
        bm.close()
