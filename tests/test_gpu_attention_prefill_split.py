"""hpa_paged_attention_prefill_split (prefill attention of fp32 pools on the bf16
matrix pipe, split operands): tests/test_gpu_attention_prefill_packed.py pointed
at the new entry -- the same poisoned pools, cases and bar (BAR = 40.8 units of
the float64 reference, through test_gpu_attention_hard's _check).  Also: two
launches agree bit for bit, rows wholly below the -10000 floor are exactly 0,
and what the kernel does not cover returns nonzero and leaves the output as it
was.

Measured worst ratios on the MI355X, six piece products per product, the same at
every page size (prefill_attn_kernel on the fp32-pool cases: 3.49):

    uniform form   1.72 (pair; uniform 0.52, hot 0.08)
    ragged form    1.04 (pair; uniform 0.49, hot 0.09)
    one row        page 8 1.26 (pair; ramp_up 0.96, ramp_down 0.89), page 64 0.98 (ramp_up; pair 0.69)
    below_floor_one and below_floor_all 0.00 (the zero output exactly zero)

With all nine piece products (every product exact; an A/B build, -DHPA_SPLIT_TERMS=9):
uniform 1.69, ragged 1.07, one row 1.08 / 1.19 -- no nearer the reference, so six it is.
"""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
from test_gpu_attention_hard import RAGGED_LENS, _check, _F, _I, _pool_id, _Set

pytestmark = pytest.mark.gpu

POOLS = [(ar.HPA_F32, P) for P in (8, 16, 32, 64)]
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
    rc = L.hpa_paged_attention_prefill_split(ctypes.cast(s.d_q.ptr, _F), ctypes.addressof(pool or s.pool.s), 0,
                                             ctypes.cast(d[0].ptr, _I), tables.shape[1], ctypes.cast(d[1].ptr, _I),
                                             ctypes.cast(d[2].ptr, _I) if row0 is not None else None,
                                             ctypes.cast(d[3].ptr, _I) if row0 is not None else None, len(lens),
                                             int(max(lens)), ctypes.cast(out.ptr, _F))
    hip.check(L.hpa_synchronize())
    return rc


@pytest.mark.parametrize("ragged", [False, True], ids=["prefill", "prefill_ragged"])
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_prefill_split(hip, pool, ragged):
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
        hip.check(_launch(hip, s, s.bt[row0], ar.PREFILL_STARTS, row0 if ragged else None, lens, d_out), "split prefill")
        outs.append(hip.from_frag(d_out.download(Rp * ar.C), R, ar.C))
    _check(s, outs[0], "prefill_split_ragged" if ragged else "prefill_split")
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("pool", [POOLS[0], POOLS[-1]], ids=_pool_id)
def test_rows_below_the_floor(hip, pool):
    """decode_cases' rows as one-row sequences at start ctx - 1 (contexts 1 .. 129: up to five
    32-key tiles): within the bar, and the rows with every key below the floor exactly 0"""
    dtype, P = pool
    s = _Set(hip, ar.decode_cases(P, dtype, launches=((4, 1),), contexts=(1, 33, 64, 129)), P, dtype)
    B = s.B
    d_out = hip.DeviceBuffer((B + 15) // 16 * 16 * ar.C * 4)
    hip.check(hip.lib().hpa_memset_async(d_out.ptr, 0xFF, d_out.nbytes))
    hip.check(_launch(hip, s, s.bt, s.cs.ctx - 1, np.arange(B), np.ones(B), d_out), "split prefill")
    got = hip.from_frag(d_out.download(d_out.nbytes // 4), B, ar.C)
    _check(s, got, "prefill_split_one_row")
    dead = np.array(s.cs.kind) == "below_floor_all"
    assert dead.any() and not got.reshape(B, ar.NH, ar.HS)[dead].any()


@pytest.mark.parametrize("field,value", [("dtype", ar.HPA_BF16), ("dtype", ar.HPA_FP8), ("page_size", 4),
                                         ("head_size", 32)])
def test_refused(hip, field, value):
    """a copy of an fp32 pool's descriptor with one field the kernel does not cover (nothing is
    launched, so nothing reads through it)"""
    s = _sets.get(((ar.HPA_F32, 16), False)) or _Set(hip, ar.prefill_cases(ar.HPA_F32), 16, ar.HPA_F32)
    d_out = hip.DeviceBuffer(16 * ar.C * 4)
    hip.check(hip.lib().hpa_memset_async(d_out.ptr, 0xFF, d_out.nbytes))
    bad = type(s.pool.s).from_buffer_copy(s.pool.s)
    setattr(bad, field, value)
    assert _launch(hip, s, s.bt[:1], [0], None, [4], d_out, pool=bad) != 0
    assert (d_out.download(16 * ar.C, np.uint32) == 0xFFFFFFFF).all()
