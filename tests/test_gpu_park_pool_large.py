"""hpa_pool_scatter_pages / hpa_pool_gather_pages on page pools of more than 2, 4
and 8 GiB per layer: the geometry, the marks and the skipping pool opener of
tests/test_gpu_pool_large.py (tests/pool_marks.py), bit equality as its bar.

The pages moved are page 0, the pool's last page and the pages either side of
every mark (where a 32-bit byte offset or element index would wrap), in a
shuffled order, so the parked buffer's order is not the pool's.  The slab is
0xFF everywhere else: a wrapped address would write into, or read from, a page
that is checked to hold poison still.
"""
import numpy as np
import pytest

import pool_marks as pm
import test_gpu_pool_large as tpl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pool", tpl.POOLS, ids=tpl._pool_id)
def test_scatter_then_gather_across_every_mark(hip, pool):
    dtype, P = pool
    big, n, pb, mk = tpl._poisoned(hip, dtype, P)
    try:
        rng = np.random.default_rng([23, int(dtype), P])
        pages = [0, n - 1]
        for m in mk:
            up = -(-m // pb)
            pages += [up - 1, up]
        tpl._assert_spread("park", dtype, P, np.array([pages], np.int64))
        for m, (lo, hi) in pm.sides(pages, pb, mk).items():
            assert lo >= 1 and hi >= 1, (m, lo, hi)
        assert big.park_bytes(len(pages)) == len(pages) * pb  # one layer
        order = rng.permutation(len(pages))
        slots = np.array(pages, np.int32)[order]
        buf = hip.PinnedBuffer(big.park_bytes(len(slots)))
        data = rng.integers(0, 255, (len(slots), pb), dtype=np.uint8)  # never 0xFF: no byte looks untouched
        buf.array[:] = data.reshape(-1)
        big.scatter_pages(slots, buf)
        hip.check(hip.lib().hpa_synchronize())
        want = {int(s): data[i] for i, s in enumerate(slots)}
        near = sorted({q for p in pages for q in range(p - 2, p + 3) if 0 <= q < n})
        for q in near:
            got = tpl._page_bytes(hip, big, q, pb)
            if q in want:
                assert np.array_equal(got, want[q]), (q, int(np.flatnonzero(got != want[q])[0]))
            else:
                assert (got == 0xFF).all(), (q, int(np.flatnonzero(got != 0xFF)[0]))
        # gather them back in another order, into device memory and into pinned memory
        order2 = rng.permutation(len(pages))
        slots2 = np.array(pages, np.int32)[order2]
        expect = np.stack([want[int(s)] for s in slots2]).reshape(-1)
        dev = hip.DeviceBuffer(buf.nbytes)
        big.gather_pages(slots2, dev)
        buf.array.fill(0xEE)
        big.gather_pages(slots2, buf)
        hip.check(hip.lib().hpa_synchronize())
        assert np.array_equal(dev.download((buf.nbytes,), np.uint8), expect)
        assert np.array_equal(buf.array, expect)
        for q in near:  # a gather writes nothing into the pool
            if q not in want:
                assert (tpl._page_bytes(hip, big, q, pb) == 0xFF).all(), q
        print(f"POOLLARGE park {tpl._pool_id(pool)} pool={n * pb / pm.GiB:.3f}GiB scattered to {slots.tolist()}, gathered "
              f"from {slots2.tolist()}, marks at pages {[m // pb for m in mk]}: byte-exact, {len(near) - len(want)} "
              f"neighbouring pages untouched")
        dev.free()
        buf.free()
    finally:
        big.destroy()
