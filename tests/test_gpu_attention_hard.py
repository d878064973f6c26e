"""Every stand-alone attention kernel against the float64 reference of
tests/attn_ref64.py, on a peaked softmax aimed at the kernels' edges and on
pools with no clean byte outside the contexts.

Decode: hpa_paged_attention_decode, _decode_frag, _decode_split and
_decode_split_w over fp32, bf16 and fp8 (per-head scales 0.5 / 2) pools,
page sizes 8..64, and (waves, splits) in attn_ref64.LAUNCHES -- 16 ranges on
short contexts leave ranges without a tile on purpose.  One batch per pool
(attn_ref64.decode_cases: hot and pair keys at 0, 1, P-1, P, 62..65, ctx-2,
ctx-1, every wave's last tile and every range edge of every launch; ramps of
300 nats in both directions; rows wholly below the -10000 floor; a uniform
control) at contexts 1 .. 1024.  Prefill: hpa_paged_attention_prefill and
_prefill_ragged at starts 0, 5, 70, 250 with up to 130 rows, hot keys at 0,
start-1, start, the row's own key, the one before, and the 16-key tile edges
below it; the ragged call has a whole 64-query block past a 5-row sequence.

Pools: the slab is 0xFF (NaN in every pool dtype) before anything is written,
the slots past a context in its last page are NaN, pages are handed out in a
random permutation and table entries past a sequence's pages are -1.  Every
output must be finite and within BAR = 8 x REF_WORST units of the reference
(tests/test_attn_ref64.py: set from the reference's own arithmetic, no
kernel's result in it): ratio = max_d |got - out| / unit_d <= 40.8.

Measured worst ratios on the MI355X (REF_WORST, the reference arithmetic
itself, is 5.1):

    decode, fp32 pool    5.55 (pair; ramp_down 4.69, ramp_up 3.70, uniform 0.59, hot 0.22)
    decode, bf16 pool    5.10 (pair; uniform 0.72, ramps 0.71)
    decode, fp8 pool     2.13 (pair; hot 1.90)
    prefill (MFMA)       5.92 (fp8 pool, pair; fp32 pool 3.49, bf16 pool 4.05)
    rows wholly below the floor: 0.00 on every kernel (the zero output exactly zero)
"""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
from test_attn_ref64 import BAR

pytestmark = pytest.mark.gpu

POOLS = [(d, P) for d in (ar.HPA_F32, ar.HPA_BF16, ar.HPA_FP8) for P in (8, 16, 32, 64)
         if P % {ar.HPA_F32: 4, ar.HPA_BF16: 8, ar.HPA_FP8: 16}[d] == 0]
DTYPE_NAME = {ar.HPA_F32: "f32", ar.HPA_BF16: "bf16", ar.HPA_FP8: "fp8"}
_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
_sets = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_sets():
    yield
    _sets.clear()


def _pool_id(p):
    return f"{DTYPE_NAME[p[0]]}-P{p[1]}"


class _Set:
    """one poisoned pool with its case batch uploaded: shared by every test of the (dtype, P);
    pool_kw: attn_ref64.poisoned_pool's further arguments (tests/test_gpu_pool_large.py)"""

    def __init__(self, hip, cs, P, dtype, **pool_kw):
        self.cs, self.P, self.dtype = cs, P, dtype
        self.pool, tables = ar.poisoned_pool(hip, cs, P, dtype, **pool_kw)
        self.tables = tables
        self.bt = np.ascontiguousarray(tables[cs.seq])  # a row's table is its sequence's (rows share pages)
        self.maxp = self.bt.shape[1]
        self.B = len(cs.seq)
        self.d_q = hip.DeviceBuffer.from_array(cs.q)
        self.d_bt = hip.DeviceBuffer.from_array(self.bt)
        self.d_pos = hip.DeviceBuffer.from_array(cs.ctx - 1)
        cs.reference()


def _decode_set(hip, dtype, P):
    if ("d", dtype, P) not in _sets:
        _sets["d", dtype, P] = _Set(hip, ar.decode_cases(P, dtype), P, dtype)
    return _sets["d", dtype, P]


def _check(s, got, what):
    r = s.cs.ratios(got)
    by = s.cs.worst_by_kind(r)
    print(f"ATTNHARD {what} {_pool_id((s.dtype, s.P))} rows={s.B} worst={r.max():.3f} "
          + " ".join(f"{k}={v:.3f}" for k, v in by.items()))
    i, h = np.unravel_index(np.argmax(r), r.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output, first at row {int(np.argwhere(~np.isfinite(got))[0][0])}"
    assert r.max() <= BAR, f"{what}: row {i} head {h} ({s.cs.kind[i][h]}, ctx {s.cs.ctx[i]}): ratio {r.max():.2f} > {BAR}"
    return float(r.max())


@pytest.mark.parametrize("frag", [False, True], ids=["decode", "decode_frag"])
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_decode(hip, pool, frag):
    L = hip.lib()
    s = _decode_set(hip, *pool)
    Mp = (s.B + 15) // 16 * 16
    d_out = hip.DeviceBuffer(Mp * ar.C * 4)
    try:
        for waves in (1, 4, 8):
            hip.check(L.hpa_memset_async(d_out.ptr, 0xFF, d_out.nbytes))
            hip.check(L.hpa_set_attention_waves(waves))
            fn = L.hpa_paged_attention_decode_frag if frag else L.hpa_paged_attention_decode
            hip.check(fn(s.d_q.ptr, s.pool.ref, 0, s.d_bt.ptr, s.maxp, s.d_pos.ptr, d_out.ptr, s.B), "decode attention")
            hip.check(L.hpa_synchronize())
            got = hip.from_frag(d_out.download(Mp * ar.C), s.B, ar.C) if frag else d_out.download((s.B, ar.C))
            _check(s, got, f"{'frag' if frag else 'decode'} waves={waves}")
    finally:
        hip.check(L.hpa_set_attention_waves(0))


@pytest.mark.parametrize("by_arg", [False, True], ids=["decode_split", "decode_split_w"])
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_decode_split(hip, pool, by_arg):
    """waves by hpa_set_attention_waves (frag output) or by the _w argument
    (row-major output); per split count one zeroed workspace, launched twice:
    bit-identical, the arrival counters zero after each launch"""
    L = hip.lib()
    s = _decode_set(hip, *pool)
    Mp = (s.B + 15) // 16 * 16
    d_out = hip.DeviceBuffer(Mp * ar.C * 4)
    ws = {}
    try:
        for waves, S in ar.LAUNCHES:
            wsb = L.hpa_attn_ws_bytes(s.B, ar.NH, S)
            if S not in ws:
                ws[S] = hip.DeviceBuffer(max(wsb, 4))
                hip.check(L.hpa_memset_async(ws[S].ptr, 0, ws[S].nbytes))
            outs = []
            for _ in range(2):
                hip.check(L.hpa_memset_async(d_out.ptr, 0xFF, d_out.nbytes))
                if by_arg:
                    hip.check(L.hpa_paged_attention_decode_split_w(s.d_q.ptr, s.pool.ref, 0, s.d_bt.ptr, s.maxp,
                                                                   s.d_pos.ptr, d_out.ptr, s.B, S,
                                                                   ws[S].ptr if wsb else None, 0, waves), "split_w")
                else:
                    hip.check(L.hpa_set_attention_waves(waves))
                    hip.check(L.hpa_paged_attention_decode_split(s.d_q.ptr, s.pool.ref, 0, s.d_bt.ptr, s.maxp,
                                                                 s.d_pos.ptr, d_out.ptr, s.B, S,
                                                                 ws[S].ptr if wsb else None, 1), "split")
                hip.check(L.hpa_synchronize())
                outs.append(d_out.download((s.B, ar.C)) if by_arg
                            else hip.from_frag(d_out.download(Mp * ar.C), s.B, ar.C))
                if wsb:
                    cnt = ws[S].download(s.B * ar.NH, np.int32, offset=s.B * ar.NH * S * 68 * 4)
                    assert not cnt.any(), (waves, S)
            _check(s, outs[0], f"{'split_w' if by_arg else 'split'} waves={waves} S={S}")
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (waves, S)
    finally:
        hip.check(L.hpa_set_attention_waves(0))


RAGGED_LENS = (130, 5, 70, 97)  # T = 130: the 5-row sequence has two whole 64-query blocks past its rows


def _prefill_set(hip, dtype, P, ragged):
    key = ("p", dtype, P, ragged)
    if key not in _sets:
        cs = ar.prefill_cases(dtype, lens=RAGGED_LENS if ragged else (130,) * 4, seed=2 if ragged else 1)
        _sets[key] = _Set(hip, cs, P, dtype)
    return _sets[key]


@pytest.mark.parametrize("ragged", [False, True], ids=["prefill", "prefill_ragged"])
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_prefill(hip, pool, ragged):
    L = hip.lib()
    dtype, P = pool
    s = _prefill_set(hip, dtype, P, ragged)
    lens = np.array(RAGGED_LENS if ragged else (130,) * 4, np.int32)
    starts = np.array(ar.PREFILL_STARTS, np.int32)
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    R = int(lens.sum())
    assert R == s.B
    Rp = (R + 15) // 16 * 16
    tables = np.ascontiguousarray(s.bt[row0])  # one table per sequence
    d_bt = hip.DeviceBuffer.from_array(tables)
    d_start = hip.DeviceBuffer.from_array(starts)
    d_out = hip.DeviceBuffer(Rp * ar.C * 4)
    hip.check(L.hpa_memset_async(d_out.ptr, 0xFF, d_out.nbytes))
    q, out = ctypes.cast(s.d_q.ptr, _F), ctypes.cast(d_out.ptr, _F)
    bt, st = ctypes.cast(d_bt.ptr, _I), ctypes.cast(d_start.ptr, _I)
    if ragged:
        d_row0, d_len = hip.DeviceBuffer.from_array(row0), hip.DeviceBuffer.from_array(lens)
        hip.check(L.hpa_paged_attention_prefill_ragged(q, ctypes.addressof(s.pool.s), 0, bt, s.maxp, st,
                                                       ctypes.cast(d_row0.ptr, _I), ctypes.cast(d_len.ptr, _I),
                                                       len(lens), int(lens.max()), out), "ragged prefill attention")
    else:
        hip.check(L.hpa_paged_attention_prefill(q, ctypes.addressof(s.pool.s), 0, bt, s.maxp, st, len(lens),
                                                int(lens[0]), out), "prefill attention")
    hip.check(L.hpa_synchronize())
    _check(s, hip.from_frag(d_out.download(Rp * ar.C), R, ar.C), "prefill_ragged" if ragged else "prefill")
