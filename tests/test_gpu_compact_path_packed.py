"""hpa_pool_compact_path_packed: a 2-layer pool of random bytes, paths across
a page edge, n_accepted = 0 and -1; the pool afterwards equals a numpy
restatement of the move, byte for byte.  An fp32 pool (dtype 0) is refused
and keeps every byte."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_I = ctypes.POINTER(ctypes.c_int)
NL, NH, HS, MR = 2, 2, 64, 8


def _p(buf):
    return ctypes.cast(buf.ptr, _I)


@pytest.mark.parametrize("dtype,P", [(0, 16), (1, 8), (1, 16), (1, 32), (1, 64), (2, 16), (2, 32), (2, 64)])
def test_compact_path_packed_moves_the_path(hip, dtype, P):
    L = hip.lib()
    rng = np.random.default_rng([5, dtype, P])
    cases = [(P - 2, [2, 5, 6]),              # destinations on both sides of the page edge, sources past it
             (P + 1, [1, 2, 3]),              # consecutive already: nothing moves
             (3, None),                       # untouched (n_accepted = -1)
             (5, []),                         # n_accepted = 0
             (P - 3, [1, 4, 5, 6, 7]),        # first in place, then a gap across the edge
             (P - 2, [7]),                    # the last node into slot 1, from the next page
             (3 * P - 8, [1, 2, 3, 4, 5, 6, 7])]
    B, pages_per = len(cases), 5
    pool = hip.Pool(NL, NH, P, B * pages_per + 2, dtype=dtype)
    elem = {hip.HPA_F32: np.uint32, hip.HPA_BF16: np.uint16, hip.HPA_FP8: np.uint8}[dtype]
    host = rng.integers(0, 256, pool.s.bytes, dtype=np.uint8).view(elem)  # any bytes: the copy is bitwise
    hip.check(L.hpa_memcpy(pool.s.base, host.ctypes.data, host.nbytes), "pool upload")
    bt = rng.permutation(B * pages_per + 2).astype(np.int32)[:B * pages_per].reshape(B, pages_per).copy()
    start = np.array([c[0] for c in cases], np.int32)
    acc = np.array([-1 if c[1] is None else len(c[1]) for c in cases], np.int32)
    path = np.full((B, MR), 99, np.int32)  # entries past a are never read
    for b, c in enumerate(cases):
        path[b, :len(c[1] or [])] = c[1] or []
    d = [hip.DeviceBuffer.from_array(a) for a in (bt, start, path, acc)]
    want, crossed = host.copy(), 0
    for b, (st, pth) in enumerate(cases):
        for k, p in enumerate(pth or [], 1):
            s, t = st + p, st + k
            crossed += p != k and s // P != t // P
            for layer in range(NL):
                for head in range(NH):
                    for dim in range(HS):
                        for index in (L.hpa_pool_k_index, L.hpa_pool_v_index):
                            want[index(pool.ref, layer, int(bt[b, t // P]), head, t % P, dim)] = \
                                host[index(pool.ref, layer, int(bt[b, s // P]), head, s % P, dim)]
    assert crossed >= 3 and not np.array_equal(want, host)
    rc = L.hpa_pool_compact_path_packed(pool.ref, _p(d[0]), pages_per, _p(d[1]), _p(d[2]), _p(d[3]), B)
    if dtype == hip.HPA_F32:
        assert rc != 0
        want = host
    else:
        hip.check(rc, "compact_path_packed")
    hip.check(L.hpa_synchronize())
    got = np.empty_like(host)
    hip.check(L.hpa_memcpy(got.ctypes.data, pool.s.base, got.nbytes), "pool download")
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, f"{diff.size} elements differ, first at {diff[:4]}"

