"""hpa_park_bytes / hpa_park_offset (include/hip_paged_attn.h): the layout of a
parked buffer against its formula.  Host arithmetic only: the pool is a
hand-filled HpaKVPool (no device, no allocation).

    page_bytes = 2 NH P hs * elem_bytes
    offset(l, i) = (l * n_pages + i) * page_bytes
    bytes        = L * n_pages * page_bytes
"""
import os
import subprocess

import pytest

import pool_marks as pm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DTYPES = (pm.F32, pm.BF16, pm.FP8)
SHAPES = [(d, P) for d in DTYPES for P in (8, 16, 64) if P % pm.MIN_PAGE[d] == 0]
N_PAGES = (1, 63, 64, 65, 130)
L, NH, HS = 3, 2, 64


@pytest.fixture(scope="module")
def pa():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "llm.c-paged_amd"), "-j8"], check=True)
    import pagedattn
    pagedattn.lib()
    return pagedattn


def shape_only_pool(pa, dtype, P, num_pages=1000, layers=L):
    s = pa.HpaKVPool()
    s.base = None
    s.num_layers, s.num_heads, s.head_size, s.page_size, s.num_pages, s.dtype = layers, NH, HS, P, num_pages, dtype
    s.elem_bytes = pm.ELEM_BYTES[dtype]
    s.page_elems = pm.page_elems(NH, P, HS)
    s.layer_elems = num_pages * s.page_elems
    s.bytes = layers * s.layer_elems * s.elem_bytes
    return s


def test_shapes_cover_every_dtype():
    assert (pm.FP8, 8) not in SHAPES and len(SHAPES) == 8 and {d for d, _ in SHAPES} == set(DTYPES)


@pytest.mark.parametrize("n_pages", N_PAGES)
@pytest.mark.parametrize("dtype,P", SHAPES)
def test_layout_is_the_formula(pa, dtype, P, n_pages):
    s = shape_only_pool(pa, dtype, P)
    pb = 2 * NH * P * HS * pm.ELEM_BYTES[dtype]
    total = pa.park_bytes(s, n_pages)
    assert total == L * n_pages * pb
    offs = [pa.park_offset(s, n_pages, l, i) for l in range(L) for i in range(n_pages)]
    assert offs == [(l * n_pages + i) * pb for l in range(L) for i in range(n_pages)]
    # strictly increasing in (layer, i), one page apart, the last page ends the buffer
    assert offs[0] == 0 and all(b - a == pb for a, b in zip(offs, offs[1:]))
    assert offs[-1] + pb == total


def test_layout_does_not_depend_on_the_pool_size(pa):
    """where the pages sat in the pool -- and how large it is -- is not in the buffer"""
    a, b = shape_only_pool(pa, pm.F32, 16, num_pages=64), shape_only_pool(pa, pm.F32, 16, num_pages=1 << 20)
    assert pa.park_bytes(a, 65) == pa.park_bytes(b, 65)
    assert pa.park_offset(a, 65, 2, 64) == pa.park_offset(b, 65, 2, 64)


def test_sizes_past_32_bits(pa):
    """64-bit arithmetic: 48 layers x 4096 pages x 384 KiB"""
    s = shape_only_pool(pa, pm.F32, 64, layers=48)
    s.num_heads, s.page_elems = 24, pm.page_elems(24, 64)
    pb = 2 * 24 * 64 * 64 * 4
    assert pa.park_bytes(s, 4096) == 48 * 4096 * pb > 1 << 36
    assert pa.park_offset(s, 4096, 47, 4095) == (47 * 4096 + 4095) * pb
