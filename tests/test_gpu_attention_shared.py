"""hpa_paged_attention_decode_shared (hpa_attn_shared.hip) against the float64
reference of tests/attn_ref64.py on the case set of tests/shared_ref64.py.

One poisoned pool per page size (8, 16, 32, 64), NH = 2, one layer: the slab
0xFF before anything is written, NaN in the slots past each context, pages
handed out in a random permutation, table entries past a sequence's pages -1.
The members of a group hold the SAME pages for the tokens they share and
their own pages from there on; the unit tables are the case set's (shared
tiles 1, 2, 5; units of 1, 2, 3 and 8 members; 9 sharers as two units over the
same pages; a unit below what two of its members share; non-members between
members by index; member positions 64t, 64t + 63, 64t + 64, 64t + 300).  Each
pool is run at prefix_splits 1, 2, 3 (three ranges over one or two tiles leave
ranges without a tile), waves 4 and 8, row-major and frag output.

The bar is the project's (tests/test_attn_ref64.py): every output finite and
ratio = max_d |got - out| / unit_d <= BAR = 40.8, every row counted; rows
wholly below the floor exactly 0.  Rows outside every unit, and every row
under an empty plan, carry the bits of hpa_paged_attention_decode_split_w at
splits = 1 and the same waves; a call repeats bit for bit; the argument
refusals of hip_paged_attn.h launch nothing.

Measured worst ratios on the MI355X (REF_WORST, the reference arithmetic
itself, is 5.1), the same at every prefix_splits, waves and layout:

    P = 64: 4.13 (pair; ramp_down 3.90, ramp_up 2.08, uniform 0.32, hot 0.04)
    rows wholly below the floor: 0.00 (the zero output exactly zero)
"""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
import shared_ref64 as sr
from test_attn_ref64 import BAR

pytestmark = pytest.mark.gpu

PAGES = (8, 16, 32, 64)
_sets = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_sets():
    yield
    _sets.clear()


class _Set:
    """the case set of one page size in a poisoned pool, tables and queries uploaded"""

    def __init__(self, hip, P):
        L = hip.lib()
        sc = self.sc = sr.shared_cases(P)
        cs = sc.cs
        self.P, self.B = P, sc.B
        npg = [(int(c) + P - 1) // P for c in cs.ctx]
        # pages: a group's shared ones (up to the largest own_from of its rows), then each row's own
        groups = sorted({int(g) for g in sc.group if g >= 0})
        g_pages = {g: int(max(sc.own_from[sc.group == g])) // P for g in groups}
        total = sum(g_pages.values()) + sum(npg[i] - int(sc.own_from[i]) // P for i in range(sc.B))
        num_pages = total + 3
        self.pool = hip.Pool(1, ar.NH, P, num_pages, dtype=ar.HPA_F32)
        hip.check(L.hpa_memset_async(self.pool.s.base, 0xFF, self.pool.s.bytes), "poison")
        hip.check(L.hpa_synchronize())
        perm = np.random.default_rng([3, P]).permutation(num_pages).astype(np.int32)
        nxt = 0
        g_list = {}
        for g in groups:
            g_list[g] = perm[nxt:nxt + g_pages[g]]
            nxt += g_pages[g]
        bt = np.full((sc.B, max(npg)), -1, np.int32)
        written = set()
        for i in range(sc.B):
            K, V = cs.seqs[i]
            own = int(sc.own_from[i]) // P
            if own:
                bt[i, :own] = g_list[int(sc.group[i])][:own]
            bt[i, own:npg[i]] = perm[nxt:nxt + npg[i] - own]
            nxt += npg[i] - own
            pad = np.full((npg[i] * P - K.shape[0], ar.C), np.nan, np.float32)
            Kp, Vp = np.concatenate([K, pad]), np.concatenate([V, pad])
            # a shared page is written once, by the first row that holds it (the others hold equal values:
            # tests/test_shared_ref64.py); own pages by their row
            todo = [lp for lp in range(npg[i]) if int(bt[i, lp]) not in written]
            for lp in todo:
                self.pool.write_tokens(0, [bt[i, lp]], Kp[lp * P:(lp + 1) * P], Vp[lp * P:(lp + 1) * P])
                written.add(int(bt[i, lp]))
        assert nxt == total
        self.bt, self.maxp = bt, bt.shape[1]
        self.max_units = max(sc.B // 2, len(sc.units))
        members, tiles, skip = sc.tables(self.max_units)
        for m, t in sc.units:  # the tables honour the kernels' invariants
            n = 64 * t // P
            for i in m:
                assert 64 * t <= sc.pos[i] and np.array_equal(bt[i, :n], bt[m[0], :n]) and (bt[i, :n] >= 0).all()
        self.d_q = hip.DeviceBuffer.from_array(cs.q)
        self.d_bt = hip.DeviceBuffer.from_array(bt)
        self.d_pos = hip.DeviceBuffer.from_array(sc.pos.astype(np.int32))
        self.d_members = hip.DeviceBuffer.from_array(members)
        self.d_tiles = hip.DeviceBuffer.from_array(tiles)
        self.d_skip = hip.DeviceBuffer.from_array(skip)
        self.d_zero_tiles = hip.DeviceBuffer.from_array(np.zeros_like(tiles))
        self.d_zero_skip = hip.DeviceBuffer.from_array(np.zeros_like(skip))
        self.Mp = (sc.B + 15) // 16 * 16
        self.d_out = hip.DeviceBuffer(self.Mp * ar.C * 4)
        self.ws = hip.DeviceBuffer(L.hpa_attn_shared_ws_bytes(sc.B, ar.NH, max(sr.SPLITS)))
        hip.check(L.hpa_memset_async(self.ws.ptr, 0xFF, self.ws.nbytes))  # nothing relies on a clean workspace
        cs.reference()

    def shared(self, hip, splits, waves, frag, empty=False, ws="own"):
        L = hip.lib()
        hip.check(L.hpa_memset_async(self.d_out.ptr, 0xFF, self.d_out.nbytes))
        rc = L.hpa_paged_attention_decode_shared(
            self.d_q.ptr, self.pool.ref, 0, self.d_bt.ptr, self.maxp, self.d_pos.ptr, self.d_out.ptr, self.B,
            self.d_members.ptr, (self.d_zero_tiles if empty else self.d_tiles).ptr, self.max_units,
            (self.d_zero_skip if empty else self.d_skip).ptr, splits, self.ws.ptr if ws == "own" else ws,
            int(frag), waves)
        hip.check(L.hpa_synchronize())
        return rc, self.download(hip, frag)

    def plain(self, hip, waves, frag):
        L = hip.lib()
        hip.check(L.hpa_memset_async(self.d_out.ptr, 0xFF, self.d_out.nbytes))
        hip.check(L.hpa_paged_attention_decode_split_w(self.d_q.ptr, self.pool.ref, 0, self.d_bt.ptr, self.maxp,
                                                       self.d_pos.ptr, self.d_out.ptr, self.B, 1, None, int(frag),
                                                       waves), "split_w")
        hip.check(L.hpa_synchronize())
        return self.download(hip, frag)

    def download(self, hip, frag):
        if frag:
            return hip.from_frag(self.d_out.download(self.Mp * ar.C), self.B, ar.C)
        return self.d_out.download((self.B, ar.C))


def _set(hip, P):
    if P not in _sets:
        _sets[P] = _Set(hip, P)
    return _sets[P]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("frag", [False, True], ids=["rows", "frag"])
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("P", PAGES)
def test_shared_against_reference(hip, P, waves, frag):
    s = _set(hip, P)
    cs = s.sc.cs
    plain = s.plain(hip, waves, frag)
    outside = s.sc.unit_of < 0
    for splits in sr.SPLITS:
        rc, got = s.shared(hip, splits, waves, frag)
        assert rc == 0
        r = cs.ratios(got)
        by = cs.worst_by_kind(r)
        print(f"SHAREDATTN P={P} waves={waves} frag={int(frag)} splits={splits} rows={s.B} worst={r.max():.3f} "
              + " ".join(f"{k}={v:.3f}" for k, v in by.items()))
        assert np.isfinite(got).all(), f"non-finite output, first at row {int(np.argwhere(~np.isfinite(got))[0][0])}"
        i, h = np.unravel_index(np.argmax(r), r.shape)
        assert r.max() <= BAR, (f"row {i} head {h} ({cs.kind[i][h]}, ctx {cs.ctx[i]}, unit {s.sc.unit_of[i]}, "
                                f"tiles {s.sc.skip[i]}): ratio {r.max():.2f} > {BAR}")
        kinds = np.array(cs.kind)
        assert not got[np.repeat(kinds == "below_floor_all", ar.HS, 1)].any()  # exactly 0
        # a row outside every unit: the present kernel's bits, whatever the other rows do
        assert np.array_equal(_bits(got[outside]), _bits(plain[outside]))
        # a call repeats bit for bit
        rc2, again = s.shared(hip, splits, waves, frag)
        assert rc2 == 0 and np.array_equal(_bits(got), _bits(again))


@pytest.mark.parametrize("P", PAGES)
def test_empty_plan_is_the_present_kernel(hip, P):
    """every unit_tiles and seq_skip 0: the bits of decode_split_w(splits = 1) at the same waves"""
    s = _set(hip, P)
    for waves in (4, 8, 1, 2):
        for frag in (False, True):
            want = s.plain(hip, waves, frag)
            rc, got = s.shared(hip, 2, waves, frag, empty=True)
            assert rc == 0 and np.array_equal(_bits(got), _bits(want)), (waves, frag)
    # no unit table at all (max_units = 0): no workspace needed
    L = hip.lib()
    hip.check(L.hpa_memset_async(s.d_out.ptr, 0xFF, s.d_out.nbytes))
    rc = L.hpa_paged_attention_decode_shared(s.d_q.ptr, s.pool.ref, 0, s.d_bt.ptr, s.maxp, s.d_pos.ptr, s.d_out.ptr,
                                             s.B, None, None, 0, s.d_zero_skip.ptr, 1, None, 0, 4)
    hip.check(L.hpa_synchronize())
    assert rc == 0 and np.array_equal(_bits(s.download(hip, False)), _bits(s.plain(hip, 4, False)))


def test_refusals_launch_nothing(hip):
    L = hip.lib()
    s = _set(hip, 16)

    def untouched():
        hip.check(L.hpa_synchronize())
        return (_bits(s.d_out.download((s.B, ar.C))) == 0xFFFFFFFF).all()

    def call(pool, splits=1, ws=None, max_units=None):
        hip.check(L.hpa_memset_async(s.d_out.ptr, 0xFF, s.d_out.nbytes))
        return L.hpa_paged_attention_decode_shared(
            s.d_q.ptr, pool, 0, s.d_bt.ptr, s.maxp, s.d_pos.ptr, s.d_out.ptr, s.B, s.d_members.ptr, s.d_tiles.ptr,
            s.max_units if max_units is None else max_units, s.d_skip.ptr, splits, s.ws.ptr if ws is None else ws, 0, 4)

    for dtype in (ar.HPA_BF16, ar.HPA_FP8):  # a pool that is not fp32
        other = hip.Pool(1, ar.NH, 16, 4, dtype=dtype)
        assert call(other.ref) != 0 and untouched()
        other.destroy()
    fake = hip.HpaKVPool()  # head size and page size: the descriptor alone decides
    ctypes.memmove(ctypes.byref(fake), ctypes.byref(s.pool.s), ctypes.sizeof(fake))
    fake.head_size = 128
    assert call(ctypes.byref(fake)) != 0 and untouched()
    ctypes.memmove(ctypes.byref(fake), ctypes.byref(s.pool.s), ctypes.sizeof(fake))
    fake.page_size = 4
    assert call(ctypes.byref(fake)) != 0 and untouched()
    for splits in (0, -1, 17):
        assert call(s.pool.ref, splits=splits) != 0 and untouched()
    assert call(s.pool.ref, ws=0) != 0 and untouched()                 # null workspace while a unit exists
    assert call(s.pool.ref, ws=s.ws.ptr + 4) != 0 and untouched()      # misaligned
    assert call(s.pool.ref) == 0 and not untouched()
