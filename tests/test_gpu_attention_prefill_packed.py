"""hpa_paged_attention_prefill_packed (prefill attention of bf16 / fp8 pools on
the bf16 matrix pipe): tests/test_gpu_attention_hard.py::test_prefill pointed at
the new entry -- the same poisoned pools, cases and bar (BAR = 40.8 units of the
float64 reference, through that file's _check).  Also: two launches agree bit
for bit, rows wholly below the -10000 floor are exactly 0, and what the kernel
does not cover returns nonzero and leaves the output as it was.

Measured worst ratios on the MI355X, three bf16 pieces for q and for P, the
same at every page size (prefill_attn_kernel on these cases: 4.05 bf16, 5.92 fp8):

    bf16 pools   uniform form 2.42, ragged 2.28 (pair; uniform 0.39, hot 0.08)
    fp8 pools    uniform form 2.63 (pair; hot 1.09), ragged 1.28 (hot; pair 0.86)
    one row      bf16 page 8 2.17 (pair; ramp_down 1.50), fp8 page 16 1.24 (pair)
    below_floor_one and below_floor_all 0.00 (the zero output exactly zero)
"""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
from test_gpu_attention_hard import RAGGED_LENS, _check, _F, _I, _pool_id, _Set

pytestmark = pytest.mark.gpu

POOLS = [(ar.HPA_BF16, P) for P in (8, 16, 32, 64)] + [(ar.HPA_FP8, P) for P in (16, 32, 64)]
_sets = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_sets():
    yield
    _sets.clear()


def _launch(hip, s, tables, starts, row0, lens, out, pool=None):
    """one call of the entry over the set's queries (row0 None: the uniform form); returns its status"""
    L = hip.lib()
    tables = np.ascontiguousarray(tables, np.int32)
    d = [hip.DeviceBuffer.from_array(np.ascontiguousarray(a, np.int32))
         for a in (tables, starts, lens if row0 is None else row0, lens)]
    rc = L.hpa_paged_attention_prefill_packed(ctypes.cast(s.d_q.ptr, _F), ctypes.addressof(pool or s.pool.s), 0,
                                              ctypes.cast(d[0].ptr, _I), tables.shape[1], ctypes.cast(d[1].ptr, _I),
                                              ctypes.cast(d[2].ptr, _I) if row0 is not None else None,
                                              ctypes.cast(d[3].ptr, _I) if row0 is not None else None, len(lens),
                                              int(max(lens)), ctypes.cast(out.ptr, _F))
    hip.check(L.hpa_synchronize())
    return rc


@pytest.mark.parametrize("ragged", [False, True], ids=["prefill", "prefill_ragged"])
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_prefill_packed(hip, pool, ragged):
    L = hip.lib()
    dtype, P = pool
    lens = np.array(RAGGED_LENS if ragged else (130,) * 4, np.int32)
    if (pool, ragged) not in _sets:
        _sets[pool, ragged] = _Set(hip, ar.prefill_cases(dtype, lens=tuple(lens), seed=2 if ragged else 1), P, dtype)
    s = _sets[pool, ragged]
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    R = int(lens.sum())
    Rp = (R + 15) // 16 * 16
    d_out = hip.DeviceBuffer(Rp * ar.C * 4)
    outs = []
    for _ in range(2):
        hip.check(L.hpa_memset_async(d_out.ptr, 0xFF, d_out.nbytes))
        hip.check(_launch(hip, s, s.bt[row0], ar.PREFILL_STARTS, row0 if ragged else None, lens, d_out), "packed prefill")
        outs.append(hip.from_frag(d_out.download(Rp * ar.C), R, ar.C))
    _check(s, outs[0], "prefill_packed_ragged" if ragged else "prefill_packed")
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("pool", [(ar.HPA_BF16, 8), (ar.HPA_FP8, 16)], ids=_pool_id)
def test_rows_below_the_floor(hip, pool):
    """decode_cases' rows as one-row sequences at start ctx - 1 (contexts 1 .. 129: up to five
    32-key tiles): within the bar, and the rows with every key below the floor exactly 0"""
    dtype, P = pool
    s = _Set(hip, ar.decode_cases(P, dtype, launches=((4, 1),), contexts=(1, 33, 64, 129)), P, dtype)
    B = s.B
    d_out = hip.DeviceBuffer((B + 15) // 16 * 16 * ar.C * 4)
    hip.check(hip.lib().hpa_memset_async(d_out.ptr, 0xFF, d_out.nbytes))
    hip.check(_launch(hip, s, s.bt, s.cs.ctx - 1, np.arange(B), np.ones(B), d_out), "packed prefill")
    got = hip.from_frag(d_out.download(d_out.nbytes // 4), B, ar.C)
    _check(s, got, "prefill_packed_one_row")
    dead = np.array(s.cs.kind) == "below_floor_all"
    assert dead.any() and not got.reshape(B, ar.NH, ar.HS)[dead].any()


@pytest.mark.parametrize("field,value", [("dtype", ar.HPA_F32), ("page_size", 4), ("head_size", 32)])
def test_refused(hip, field, value):
    """a copy of a bf16 pool's descriptor with one field the kernel does not cover (nothing is
    launched, so nothing reads through it); an fp8 pool of page 8 likewise"""
    s = _sets.get(((ar.HPA_BF16, 16), False)) or _Set(hip, ar.prefill_cases(ar.HPA_BF16), 16, ar.HPA_BF16)
    d_out = hip.DeviceBuffer(16 * ar.C * 4)
    hip.check(hip.lib().hpa_memset_async(d_out.ptr, 0xFF, d_out.nbytes))
    for changes in ({field: value}, {"dtype": ar.HPA_FP8, "page_size": 8}):
        bad = type(s.pool.s).from_buffer_copy(s.pool.s)
        for k, v in changes.items():
            setattr(bad, k, v)
        assert _launch(hip, s, s.bt[:1], [0], None, [4], d_out, pool=bad) != 0
    assert (d_out.download(16 * ar.C, np.uint32) == 0xFFFFFFFF).all()
