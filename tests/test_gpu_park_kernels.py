"""hpa_pool_gather_pages / hpa_pool_scatter_pages (hpa_park.hip): whole pages of
every layer between the pool and one contiguous buffer, bit for bit.

Stand-alone pools of L = 3 layers, NH = 2, every dtype at its smallest page
size and at P = 64, 160 pages, the slab filled with random bytes the host
keeps a copy of.  n_pages in {1, 63, 64, 65, 130}: one launch, the launch edge
(HPA_PARK_MAX_PAGES = 64) from both sides, three launches.  The buffer is
device memory or pinned host memory.  Everything is compared as bytes.
"""
import numpy as np
import pytest

import pool_marks as pm

pytestmark = pytest.mark.gpu

L, NH, PAGES = 3, 2, 160
POOLS = [(d, P) for d in (pm.F32, pm.BF16, pm.FP8) for P in (pm.MIN_PAGE[d], 64)]
N_PAGES = (1, 63, 64, 65, 130)
_sets = {}


def _pool_id(p):
    return f"{ {pm.F32: 'f32', pm.BF16: 'bf16', pm.FP8: 'fp8'}[p[0]] }-P{p[1]}"


@pytest.fixture(scope="module", autouse=True)
def _drop_sets():
    yield
    for pool, _ in _sets.values():
        pool.destroy()
    _sets.clear()


def slab(hip, pool):
    out = np.empty(pool.s.bytes, np.uint8)
    hip.check(hip.lib().hpa_synchronize())
    hip.check(hip.lib().hpa_memcpy(out.ctypes.data, pool.s.base, out.nbytes), "pool download")
    return out.reshape(pool.s.num_layers, pool.s.num_pages, -1)


def source(hip, dtype, P):
    """(pool, host copy [L][PAGES][page bytes]): random bytes everywhere"""
    if (dtype, P) not in _sets:
        pool = hip.Pool(L, NH, P, PAGES, dtype=dtype)
        host = np.random.default_rng([5, int(dtype), P]).integers(0, 256, pool.s.bytes, dtype=np.uint8)
        hip.check(hip.lib().hpa_memcpy(pool.s.base, host.ctypes.data, host.nbytes), "slab upload")
        _sets[(dtype, P)] = (pool, host.reshape(L, PAGES, -1))
        assert host.size == L * PAGES * 2 * NH * P * 64 * pm.ELEM_BYTES[dtype]
    return _sets[(dtype, P)]


def arranged(hip, pool, host, slots):
    """the parked buffer the layout prescribes, from the host copy and hpa_park_offset"""
    n, pb = len(slots), host.shape[2]
    want = np.zeros(pool.park_bytes(n), np.uint8)
    for l in range(L):
        for i, s in enumerate(slots):
            o = pool.park_offset(n, l, i)
            want[o:o + pb] = host[l, s]
    return want


def download(hip, buf, n):
    hip.check(hip.lib().hpa_synchronize())
    return buf.download((n,), np.uint8) if isinstance(buf, hip.DeviceBuffer) else buf.array.copy()


def make_buffer(hip, where, nbytes):
    return hip.DeviceBuffer(nbytes) if where == "device" else hip.PinnedBuffer(nbytes)


@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("n_pages", N_PAGES)
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_gather(hip, pool, n_pages, where):
    dtype, P = pool
    src, host = source(hip, dtype, P)
    slots = np.random.default_rng([7, n_pages, P]).permutation(PAGES)[:n_pages].astype(np.int32)
    nbytes = src.park_bytes(n_pages)
    assert nbytes == L * n_pages * host.shape[2]
    buf = make_buffer(hip, where, nbytes)
    if where == "device":
        hip.check(hip.lib().hpa_memset_async(buf.ptr, 0xEE, nbytes))
    else:
        buf.array.fill(0xEE)
    src.gather_pages(slots, buf)
    got = download(hip, buf, nbytes)
    want = arranged(hip, src, host, slots)
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    assert np.array_equal(slab(hip, src), host)  # the pool itself untouched
    buf.free()


@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("n_pages", N_PAGES)
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_scatter_and_round_trip(hip, pool, n_pages, where):
    """scatter into a disjoint random set of slots of a 0xFF-poisoned second pool:
    the named pages equal the buffer's in every layer, every other byte is
    still 0xFF; gathering them again returns the buffer (gather o scatter o
    gather is the identity)"""
    dtype, P = pool
    src, host = source(hip, dtype, P)
    rng = np.random.default_rng([9, n_pages, P])
    from_slots = rng.permutation(PAGES)[:n_pages].astype(np.int32)
    to_slots = rng.permutation(PAGES)[:n_pages].astype(np.int32)
    nbytes = src.park_bytes(n_pages)
    buf = make_buffer(hip, where, nbytes)
    src.gather_pages(from_slots, buf)
    first = download(hip, buf, nbytes)
    dst = hip.Pool(L, NH, P, PAGES, dtype=dtype)
    hip.check(hip.lib().hpa_memset_async(dst.s.base, 0xFF, dst.s.bytes), "poison")
    dst.scatter_pages(to_slots, buf)
    got = slab(hip, dst)
    want = np.full_like(host, 0xFF)
    want[:, to_slots] = host[:, from_slots]
    assert np.array_equal(got, want), np.argwhere(got != want)[0].tolist()
    buf2 = make_buffer(hip, where, nbytes)
    dst.gather_pages(to_slots, buf2)
    again = download(hip, buf2, nbytes)
    assert np.array_equal(again, first)
    for b in (buf, buf2):
        b.free()
    dst.destroy()


@pytest.mark.parametrize("pool", [POOLS[0], POOLS[-1]], ids=_pool_id)
def test_refusals_launch_nothing(hip, pool):
    dtype, P = pool
    src, host = source(hip, dtype, P)
    nbytes = src.park_bytes(4)
    dev, pin = hip.DeviceBuffer(nbytes), hip.PinnedBuffer(nbytes)
    hip.check(hip.lib().hpa_memset_async(dev.ptr, 0xEE, nbytes))
    pin.array.fill(0xEE)
    pageable = np.full(nbytes + 64, 0xEE, np.uint8)
    pageable_ptr = (pageable.ctypes.data + 15) // 16 * 16
    for buf in (dev, pin):
        for slots in ([], [0, 1, PAGES, 2], [0, -1, 1, 2]):
            with pytest.raises(RuntimeError):
                src.gather_pages(slots, buf)
            with pytest.raises(RuntimeError):
                src.scatter_pages(slots, buf)
        with pytest.raises(RuntimeError):
            src.scatter_pages([3, 5, 3, 6], buf)  # a slot listed twice
        src.gather_pages([3, 3, 3, 3], buf)  # reading a page twice is fine
        src.gather_pages([0, 1, 2, 3], buf)
    for call in (src.gather_pages, src.scatter_pages):
        with pytest.raises(RuntimeError):
            call([0, 1, 2, 3], pageable_ptr)
        with pytest.raises(RuntimeError):
            call([0, 1, 2, 3], 0)
    assert np.array_equal(slab(hip, src), host)
    assert (pageable == 0xEE).all()
    want = arranged(hip, src, host, [0, 1, 2, 3])
    assert np.array_equal(download(hip, dev, nbytes), want) and np.array_equal(download(hip, pin, nbytes), want)
    dev.free()
    pin.free()


def test_nontemporal_forms_move_the_same_bytes(hip):
    """hpa_park_set_nontemporal: each of the four kernel forms, bit equal"""
    src, host = source(hip, pm.F32, 8)
    slots = np.array([7, 150, 0, 66, 159], np.int32)
    nbytes = src.park_bytes(len(slots))
    want = arranged(hip, src, host, slots)
    dst = hip.Pool(L, NH, 8, PAGES, dtype=pm.F32)
    default = hip.lib().hpa_park_nontemporal()
    try:
        for mask in (1, 2, 3, 0):
            hip.check(hip.lib().hpa_park_set_nontemporal(mask))
            assert hip.lib().hpa_park_nontemporal() == mask
            buf = hip.PinnedBuffer(nbytes)
            src.gather_pages(slots, buf)
            assert np.array_equal(download(hip, buf, nbytes), want), mask
            hip.check(hip.lib().hpa_memset_async(dst.s.base, 0xFF, dst.s.bytes), "poison")
            dst.scatter_pages(slots, buf)
            got = slab(hip, dst)
            ref = np.full_like(host, 0xFF)
            ref[:, slots] = host[:, slots]
            assert np.array_equal(got, ref), mask
            buf.free()
        assert hip.lib().hpa_park_set_nontemporal(4) != 0
    finally:
        hip.lib().hpa_park_set_nontemporal(default)
        dst.destroy()
