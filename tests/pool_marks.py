"""Where a K/V page lies from its layer's base, the offsets at which a 32-bit
form of that address would wrap (the marks), the pages a big-pool test puts
its sequences on, and deliberately 32-bit models of the tile offset.  Python
integers and numpy only; shared by tests/test_pool_index_host.py (no GPU) and
tests/test_gpu_pool_large.py.

The pool layout (include/hip_paged_attn.h): page `page` of a layer starts
page * page_elems elements from the layer's base, page_elems = 2 NH P hs.

Marks, as byte offsets from the layer's base:

    2^31 B, 2^32 B          a signed / unsigned 32-bit byte offset wraps
    2^31 eb, 2^32 eb B      a signed / unsigned 32-bit element index wraps
                            (eb = bytes per element: `int page * page_elems`)

MODELS are the four wrong answers: the tile's byte offset formed in that
32-bit type.  Each equals the true offset below its mark and differs from it
at every page that starts at or above the mark (the wrap subtracts a multiple
of 2^32 bytes or elements), which tests/test_pool_index_host.py asserts for
the very pages the GPU tests use.
"""
import numpy as np

GiB = 1 << 30
MiB = 1 << 20
F32, BF16, FP8 = 0, 1, 2
ELEM_BYTES = {F32: 4, BF16: 2, FP8: 1}
K_CHUNK = {F32: 4, BF16: 8, FP8: 16}
MIN_PAGE = {F32: 8, BF16: 8, FP8: 16}  # the smallest page size every attention kernel takes
# bytes per layer of the stand-alone pools (tests/test_gpu_pool_large.py, one layer)
BIG_LAYER_BYTES = {F32: 8 * GiB + 64 * MiB, BF16: 8 * GiB + 64 * MiB, FP8: 4 * GiB + 64 * MiB}
ENGINE_LAYER_BYTES = 4 * GiB + 64 * MiB  # the engine's big pool, per layer (two layers)


def page_elems(NH, P, hs=64):
    return 2 * NH * P * hs


def engine_pages(page_bytes):
    """pages of the engine's big pool: ENGINE_LAYER_BYTES per layer, rounded
    down to a multiple of 16 (the engine maps its manager's pages to pool slots
    in groups of up to 16 and leaves a tail in place; without one the pool's
    last slot is mapped like any other)"""
    return ENGINE_LAYER_BYTES // page_bytes // 16 * 16


def marks(layer_bytes, eb):
    """sorted byte offsets inside a layer of layer_bytes at which a 32-bit byte or element offset wraps"""
    return sorted(m for m in {1 << 31, 1 << 32, eb << 31, eb << 32} if m < layer_bytes)


def _wrap(x, signed):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if signed and x >= (1 << 31) else x


# name -> (threshold in bytes for element size eb, byte offset of `page`'s start as that type forms it)
MODELS = {
    "byte_i32": (lambda eb: 1 << 31, lambda page, pe, eb: _wrap(page * pe * eb, True)),
    "byte_u32": (lambda eb: 1 << 32, lambda page, pe, eb: _wrap(page * pe * eb, False)),
    "elem_i32": (lambda eb: eb << 31, lambda page, pe, eb: _wrap(page * pe, True) * eb),
    "elem_u32": (lambda eb: eb << 32, lambda page, pe, eb: _wrap(page * pe, False) * eb),
}


def zones(num_pages, page_bytes, layer_marks):
    """[(first page, step)]: the pool's start upward, below each mark downward,
    from each mark upward, the pool's end downward.  `From a mark upward`
    starts at the first page that begins at or above it; `below` at the page
    before that one (which holds the mark itself when the mark is not
    page-aligned)."""
    z = [(0, 1)]
    for m in layer_marks:
        up = -(-m // page_bytes)
        z += [(up - 1, -1), (up, 1)]
    z.append((num_pages - 1, -1))
    return z


def candidates(num_pages, page_bytes, layer_marks, need, least=16):
    """page indices for `need` pages, most wanted first: the k-th page of
    every zone before the (k+1)-th of any, n = max(least, need / zones
    rounded up) per zone -- the same number on each side of every mark.  The
    first 2 (marks + 1) entries are page 0, the pages either side of every
    mark and the last page, so any need >= that uses them all."""
    z = zones(num_pages, page_bytes, layer_marks)
    n = max(least, -(-need // len(z)))
    out = [p0 + k * step for k in range(n) for p0, step in z]
    assert len(set(out)) == len(out) and min(out) >= 0 and max(out) < num_pages, "zones overlap: pool too small"
    return np.array(out, np.int64)


def sides(pages, page_bytes, layer_marks):
    """{mark: (pages wholly below it, pages starting at or above it)} of the pages in use"""
    pages = np.unique(np.asarray(pages, np.int64))
    pages = pages[pages >= 0]
    return {m: (int(((pages + 1) * page_bytes <= m).sum()), int((pages * page_bytes >= m).sum())) for m in layer_marks}


def describe(pages, page_bytes, layer_marks, width=3):
    """one line: the pages in use nearest each mark, for a test's output"""
    pages = np.unique(np.asarray(pages, np.int64))
    pages = pages[pages >= 0]
    parts = [f"first {pages[:width].tolist()}"]
    for m in layer_marks:
        lo, hi = pages[pages * page_bytes < m], pages[pages * page_bytes >= m]
        parts.append(f"2^{np.log2(m):.0f}B: {lo[-width:].tolist()} | {hi[:width].tolist()}")
    parts.append(f"last {pages[-width:].tolist()}")
    return "; ".join(parts)
