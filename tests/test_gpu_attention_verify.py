"""hpa_paged_attention_verify (the few-row attention of a speculative verify
pass, hpa_verify.hip) against the float64 reference of tests/attn_ref64.py on
poisoned pools: every byte outside the contexts is 0xFF (a NaN), so a read
past a row's keys shows as a non-finite output or a ratio far above the bar.

Five sequences, fp32 pools of page size 8, 16, 32 and 64:
    start    0: 8 rows -- row 0 on an empty cache (one key)
    start    5: 1 row
    start   60: 3 rows -- positions 60..62, below the 64-token tile edge
    start  250: 8 rows
    start 1016: 8 rows -- the last ends at ctx 1024
    (a second set: start 60, 8 rows: positions 60..67 straddle the tile edge)
Hot rows aim at their own key and the one before it (the causal edge between
the rows of one pass), at key 0 and at the start.  The pass rule is the
project's: every output finite and ratio <= BAR (tests/test_attn_ref64.py).

Measured worst ratios on the MI355X (the ATTNVERIFY lines this file prints):
in the docstring of test_verify_against_float64."""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
from test_attn_ref64 import BAR

pytestmark = pytest.mark.gpu

PAGES = (8, 16, 32, 64)
STARTS = (0, 5, 60, 250, 1016)
LENS = (8, 1, 3, 8, 8)
EDGE_STARTS = (60, 1000, 7)   # second batch: a skipped sequence between two others
EDGE_LENS = (8, 0, 4)
_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
_sets = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_sets():
    yield
    _sets.clear()


class _Set:
    """a case batch in a poisoned pool of page size P, its tables uploaded;
    pool_kw: callable(cs) -> attn_ref64.poisoned_pool's further arguments (tests/test_gpu_pool_large.py)"""

    def __init__(self, hip, starts, lens, P, dtype=ar.HPA_F32, seed=3, pool_kw=None):
        # a len = 0 sequence still owns a context (one row's worth) in the pool, so its table is real
        self.cs = ar.prefill_cases(dtype, starts=starts, lens=tuple(max(n, 1) for n in lens), seed=seed)
        self.lens = np.array(lens, np.int32)
        self.starts = np.array(starts, np.int32)
        self.row0 = np.concatenate([[0], np.cumsum(np.maximum(self.lens, 1))[:-1]]).astype(np.int32)
        self.R = len(self.cs.seq)
        self.Rp = (self.R + 15) // 16 * 16
        self.P = P
        self.pool, tables = ar.poisoned_pool(hip, self.cs, P, dtype, **(pool_kw(self.cs) if pool_kw else {}))
        self.tables = tables
        self.maxp = tables.shape[1]
        self.d_q = hip.DeviceBuffer.from_array(self.cs.q)
        self.d_bt = hip.DeviceBuffer.from_array(np.ascontiguousarray(tables))
        self.d_start = hip.DeviceBuffer.from_array(self.starts)
        self.d_row0 = hip.DeviceBuffer.from_array(self.row0)
        self.d_len = hip.DeviceBuffer.from_array(self.lens)
        self.d_out = hip.DeviceBuffer(self.Rp * ar.C * 4)
        self.cs.reference()

    def launch(self, hip, T=None, fill=True):
        """one launch into the 0xFF-filled output; returns (rc, rows (R, C), raw bits)"""
        L = hip.lib()
        if fill:
            hip.check(L.hpa_memset_async(self.d_out.ptr, 0xFF, self.d_out.nbytes))
        c = ctypes.cast
        rc = L.hpa_paged_attention_verify(c(self.d_q.ptr, _F), ctypes.addressof(self.pool.s), 0, c(self.d_bt.ptr, _I),
                                          self.maxp, c(self.d_start.ptr, _I), c(self.d_row0.ptr, _I),
                                          c(self.d_len.ptr, _I), len(self.lens),
                                          int(self.lens.max()) if T is None else T, c(self.d_out.ptr, _F))
        hip.check(L.hpa_synchronize())
        raw = self.d_out.download(self.Rp * ar.C)
        return rc, hip.from_frag(raw, self.R, ar.C), raw.view(np.uint32).copy()


def _set(hip, name, P, dtype=ar.HPA_F32):
    key = (name, P, dtype)
    if key not in _sets:
        starts, lens = (STARTS, LENS) if name == "main" else (EDGE_STARTS, EDGE_LENS)
        _sets[key] = _Set(hip, starts, lens, P, dtype)
    return _sets[key]


@pytest.mark.parametrize("P", PAGES)
def test_verify_against_float64(hip, P):
    """every row of the five sequences within the bar, twice bit for bit.

    Measured worst ratio per kind (MI355X; the same for P = 8, 16, 32, 64,
    whose arithmetic is identical): uniform 0.706, hot 0.019, pair 3.256; the
    edge set of the next test: 1.241"""
    s = _set(hip, "main", P)
    assert s.R == sum(LENS)
    L = hip.lib()
    try:
        for waves in (0, 4, 8):  # by shape (8 for this small grid), then both workgroup sizes by name
            hip.check(L.hpa_set_attention_waves(waves))
            assert L.hpa_attention_waves() == waves
            rc, got, bits = s.launch(hip)
            assert rc == 0
            r = s.cs.ratios(got)
            by = s.cs.worst_by_kind(r)
            print(f"ATTNVERIFY P={P} waves={waves} rows={s.R} worst={r.max():.3f} "
                  + " ".join(f"{k}={v:.3f}" for k, v in by.items()))
            assert np.isfinite(got).all(), f"non-finite output, first at row {int(np.argwhere(~np.isfinite(got))[0][0])}"
            i, h = np.unravel_index(np.argmax(r), r.shape)
            assert r.max() <= BAR, (f"waves {waves} row {i} head {h} ({s.cs.kind[i][h]}, ctx {s.cs.ctx[i]}): "
                                    f"ratio {r.max():.2f} > {BAR}")
            rc2, _, bits2 = s.launch(hip)
            assert rc2 == 0 and np.array_equal(bits, bits2), "two launches on the same inputs differ"
    finally:
        hip.check(L.hpa_set_attention_waves(0))


@pytest.mark.parametrize("P", PAGES)
def test_verify_skips_a_len0_sequence_and_straddles_the_tile_edge(hip, P):
    """positions 60..67 (both sides of the 64-token tile edge), a len = 0
    sequence whose output row keeps its 0xFF fill, a 4-row sequence after it"""
    s = _set(hip, "edge", P)
    rc, got, _ = s.launch(hip)
    assert rc == 0
    live = np.ones(s.R, bool)
    live[s.row0[1]] = False  # the skipped sequence's one placeholder row
    assert (got[~live].view(np.uint32) == 0xFFFFFFFF).all(), "a len = 0 sequence's output row was written"
    r = s.cs.ratios(got)[live]
    print(f"ATTNVERIFY edge P={P} worst={r.max():.3f}")
    assert np.isfinite(got[live]).all()
    assert r.max() <= BAR
    # rows past the last sequence's 4 (the padding of the frag layout) stay untouched too
    _, _, bits = s.launch(hip)
    pad = hip.from_frag(bits.view(np.float32), s.Rp, ar.C)[s.R:]
    assert (pad.view(np.uint32) == 0xFFFFFFFF).all()


def test_verify_refuses_nine_rows_and_other_pools(hip):
    """T = 9, a bf16 pool and an fp8 pool: nonzero, nothing launched (the
    output keeps its fill)"""
    s = _set(hip, "main", 16)
    rc, _, bits = s.launch(hip, T=9)
    assert rc != 0 and (bits == 0xFFFFFFFF).all()
    rc, _, bits = s.launch(hip, T=0)
    assert rc != 0 and (bits == 0xFFFFFFFF).all()
    for dtype in (ar.HPA_BF16, ar.HPA_FP8):
        o = _Set(hip, EDGE_STARTS, EDGE_LENS, 16, dtype)
        rc, _, bits = o.launch(hip)
        assert rc != 0 and (bits == 0xFFFFFFFF).all(), dtype
