"""hpa_decode_chain_b16 / hpa_decode_chain_b16_first launched directly on
buffers the test owns, every phase held to float64 on the kernel's own input
to it (tests/chain_ref64.py; its CPU self-test is tests/test_chain_ref64.py).

Each case: a 3-layer pool (the launch writes layer 1, the first launch layer
0; the others must stay as they were) filled with 0xFF bytes, 4 pages per
sequence and 16 that nobody owns, a block table of stride 7 with permuted page
ids and -1 in the unused entries, ragged positions (ref64.ragged_positions,
check_position_mix); res2, fch, q_out, slab and stats_out filled with a NaN
sentinel, a guard of 64 words after every buffer; counters zero.  After the
launch: phases B, C, D, E (and the LNf statistics of a last layer) against
float64, padded rows, the whole pool before against after, the counter block,
*err, the guards.  One line per case:

  CHAINB16 <case>: B <r> C <r> D <r> [E <r> | stats <r>] |S| <LN2> <LN1>

with r the worst ratio to the phase's bound and |S| the largest ambiguous set
of a row.  Measured on the MI355X (gfx950, 256 CUs):

  B=1   P=16 f32  last=0: B 0.006 C 0.604 D 0.039 E 0.007     |S| 13 18
  B=40  P=8  bf16 last=0: B 0.040 C 0.804 D 0.331 E 0.032     |S| 21 22
  B=72  P=64 f32  last=0: B 0.040 C 0.804 D 0.331 E 0.053     |S| 21 22
  B=200 P=32 bf16 last=0: B 0.040 C 0.819 D 0.350 E 0.052     |S| 25 23
  B=256 P=8  bf16 last=0: B 0.040 C 0.819 D 0.355 E 0.052     |S| 27 26
  B=40  P=16 f32  last=1: B 0.040 C 0.804 D 0.331 stats 0.033 |S| 21 -
  B=256 P=8  bf16 last=1: B 0.040 C 0.819 D 0.355 stats 0.033 |S| 27 -
  first B=1   P=8  f32 : E 0.024 |S| - 19
  first B=40  P=16 bf16: E 0.054 |S| - 22
  first B=256 P=8  bf16: E 0.062 |S| - 26

Every case passes; repeat launches and the rows of B = 40 inside B = 200 are
bit-identical.  The whole file runs in under 3 s.

Phase C's allowance is centred on rb_lo(LN2), so an operand that legally
rounds to rb_hi spends up to the whole flip: ratios near 1 are what a correct
kernel gives there (the numpy emulation: 0.80).
"""
import ctypes

import numpy as np
import pytest

import chain_ref64 as cr

pytestmark = pytest.mark.gpu

C = cr.C
SEED = 5
GUARD = 64  # words
CHAIN_CASES = [(1, 16, "f32", 0), (40, 8, "bf16", 0), (72, 64, "f32", 0), (200, 32, "bf16", 0),
               (256, 8, "bf16", 0), (40, 16, "f32", 1), (256, 8, "bf16", 1)]
FIRST_CASES = [(1, 8, "f32"), (40, 16, "bf16"), (256, 8, "bf16")]


class Buf:
    """a device buffer of n 32-bit words and GUARD more, all filled with `fill`
    (or holding `content`)"""

    def __init__(self, hip, n=None, content=None, fill=cr.SENT32):
        if content is not None:
            content = np.ascontiguousarray(content).view(np.uint32).ravel()
            n = content.size
        self.n, self.fill = int(n), fill
        host = np.full(self.n + GUARD, fill, np.uint32)
        if content is not None:
            host[:self.n] = content
        self.d = hip.DeviceBuffer.from_array(host)
        self.ptr = self.d.ptr

    def get(self, dtype=np.float32):
        """(content as dtype, guard words)"""
        w = self.d.download(self.n + GUARD, np.uint32)
        return w[:self.n].view(dtype), w[self.n:]


@pytest.fixture(scope="module")
def weights(hip):
    """the four matrices packed to the bf16 frag layout on the device, biases and
    LayerNorm parameters; shared by every case (make_inputs gives every B the same)"""
    L = hip.lib()
    base = cr.make_inputs(256, SEED)
    dev = {}
    for name in ("w_ap", "w_fc", "w_fp", "w_qkv"):
        n, k = base[name].shape
        src = hip.DeviceBuffer.from_array(base[name])
        dst = hip.DeviceBuffer(L.hpa_frag_bf16_elems(n, k) * 2)
        hip.check(L.hpa_pack_frag_bf16(src.ptr, n, k, k, dst.ptr), "pack bf16")
        hip.check(L.hpa_synchronize())
        dev[name] = dst
    for name in ("b_ap", "b_fc", "b_fp", "b_qkv", "ln1_w", "ln1_b", "ln2_w", "ln2_b"):
        dev[name] = hip.DeviceBuffer.from_array(base[name])
    return dev


def _pool_image(hip, pool, geom):
    img = np.empty(geom["L"] * geom["layer_elems"], np.uint16 if geom["bf16"] else np.uint32)
    assert img.nbytes == pool.s.bytes
    hip.check(hip.lib().hpa_memcpy(img.ctypes.data, pool.s.base, img.nbytes), "pool download")
    return img


_RUNS = {}
_SHARED = (40, 8, "bf16", 0, False)  # the one launch three tests look at (the others' pool images are not kept)


def _launch(hip, weights, B, P, pool_t, last=0, first=False, cache=True):
    """one launch on fresh buffers; returns (inp, pg, geom, out) for chain_ref64.check_launch"""
    key = (B, P, pool_t, last, first)
    if cache and key in _RUNS:
        return _RUNS[key]
    L = hip.lib()
    if not L.hpa_decode_chain_b16_eligible(B, 768, 12):
        pytest.skip("the bf16 chain does not apply on this device (a unit per workgroup)")
    bf16 = pool_t == "bf16"
    inp = cr.make_inputs(B, SEED)
    pg = cr.make_paging(B, P)
    inp["wpe"] = inp["wpe"][:int(pg["pos"].max()) + 1]  # the largest position is the table's last row
    Mp = inp["Mp"]
    geom = cr.pool_geom(3, pg["pages"], P, bf16)
    pool = hip.Pool(3, 12, P, pg["pages"], dtype=hip.HPA_BF16 if bf16 else hip.HPA_F32)
    assert (pool.s.page_elems, pool.s.layer_elems) == (geom["page_elems"], geom["layer_elems"])
    hip.check(L.hpa_memset_async(pool.s.base, 0xFF, pool.s.bytes), "pool fill")
    hip.check(L.hpa_synchronize())
    sizes = (ctypes.c_size_t * 2)()
    hip.check(L.hpa_decode_chain_b16_sizes(B, sizes), "sizes")
    assert sizes[1] == cr.K_LINES * cr.K_PAD
    stats_mp = Mp + 16 if B == 256 else Mp  # a stride of its own, and the default
    b = dict(res2=Buf(hip, Mp * C), fch=Buf(hip, Mp * 4 * C // 2), q=Buf(hip, Mp * C), slab=Buf(hip, sizes[0]),
             stats=Buf(hip, C // 16 * stats_mp * 2), ctr=Buf(hip, sizes[1], fill=0), err=Buf(hip, 2, fill=0),
             att=Buf(hip, content=hip.to_frag(inp["att"])), bt=Buf(hip, content=pg["bt"]),
             pos=Buf(hip, content=pg["pos"]))
    b["res"] = Buf(hip, Mp * C) if first else Buf(hip, content=hip.to_frag(inp["res"]))
    a = hip.HpaChainB16Args()
    a.B, a.layer, a.last = B, 0, last
    a.pool = ctypes.pointer(pool.s)
    a.block_table, a.bt_stride, a.pos = b["bt"].ptr, pg["bt"].shape[1], b["pos"].ptr
    a.att, a.res, a.res2, a.fch = b["att"].ptr, b["res"].ptr, b["res2"].ptr, b["fch"].ptr
    for name in ("w_ap", "w_fc", "w_fp", "b_ap", "ln2_w", "ln2_b", "b_fc", "b_fp"):
        setattr(a, name, weights[name].ptr)
    if not last:
        for name in ("w_qkv", "ln1_w", "ln1_b", "b_qkv"):
            setattr(a, name, weights[name].ptr)
        a.q_out = b["q"].ptr
    if last:
        a.stats_out, a.stats_mp = b["stats"].ptr, 0 if stats_mp == Mp else stats_mp
    a.slab, a.counters, a.err, a.err_sticky = b["slab"].ptr, b["ctr"].ptr, b["err"].ptr, b["err"].ptr + 4
    before = _pool_image(hip, pool, geom)
    assert np.all(before == (0xFFFF if bf16 else 0xFFFFFFFF))
    zero_words = 1024
    if first:
        b["tok"] = Buf(hip, content=inp["tokens"])
        b["wte"], b["wpe"] = Buf(hip, content=inp["wte"]), Buf(hip, content=inp["wpe"])
        b["zero"] = Buf(hip, zero_words, fill=0xFFFFFFFF)
        hip.check(L.hpa_decode_chain_b16_first(ctypes.byref(a), b["tok"].ptr, b["wte"].ptr, b["wpe"].ptr,
                                               b["zero"].ptr, zero_words * 4), "chain b16 first")
    else:
        hip.check(L.hpa_decode_chain_b16(ctypes.byref(a)), "chain b16")
    hip.check(L.hpa_synchronize())
    out, guards = {}, {}
    for name in ("res2", "res", "q", "slab", "stats", "att", "bt", "pos"):
        out[name], g = b[name].get()
        guards[name + " guard"] = (g, cr.SENT32)
    out["q"] = out["q"].reshape(Mp, C)
    out["fch"], g = b["fch"].get(np.uint16)
    guards["fch guard"] = (g, cr.SENT32)
    out["ctr"], g = b["ctr"].get(np.int32)
    guards["counter guard"] = (g, 0)
    err, g = b["err"].get(np.int32)
    out["err"], out["err_sticky"] = int(err[0]), int(err[1])
    guards["err guard"] = (g, 0)
    # inputs the launch only reads
    for name, want in (("att", hip.to_frag(inp["att"])), ("bt", pg["bt"]), ("pos", pg["pos"])):
        guards[name + " unchanged"] = (out[name].view(np.uint32) ^ np.ravel(want).view(np.uint32), 0)
    if first or last:  # phases that do not run leave their outputs alone
        for name in (("res2", "fch", "slab", "stats") if first else ()) + (("q",) if last else ()):
            guards[name + " untouched"] = (np.asarray(out[name]).view(np.uint32), cr.SENT32)
    if first:
        z, g = b["zero"].get(np.uint32)
        out["zero"], out["zero_words"] = np.concatenate([z, g]), zero_words
        guards["counters untouched"] = (out["ctr"], 0)
    if not last and not first:
        guards["stats untouched"] = (out["stats"].view(np.uint32), cr.SENT32)
    out["stats"], out["stats_mp"] = (out["stats"], stats_mp) if last else (None, 0)
    out["guards"] = guards
    out["pool_before"], out["pool_after"] = before, _pool_image(hip, pool, geom)
    pool.destroy()
    run = (inp, pg, geom, out)
    if cache and key == _SHARED:
        _RUNS[key] = run
    return run


def _line(tag, ratios):
    keys = [k for k in ("B", "C", "D", "E", "stats") if k in ratios]
    return (f"CHAINB16 {tag}: " + " ".join(f"{k} {ratios[k]:.3f}" for k in keys)
            + f" |S| {ratios.get('S2', '-')} {ratios.get('S1', '-')}")


def test_from_frag_bf16_inverts_the_device_pack(hip):
    """from_frag_bf16(hpa_pack_frag_bf16(W)) == round_bf16(W), bit for bit"""
    L = hip.lib()
    rng = np.random.default_rng(11)
    for n, k in ((768, 768), (768, 3072)):
        W = rng.standard_normal((n, k)).astype(np.float32)
        W[0, :4] = [4.015625, 4.046875, -0.0, 2.0 ** -126]  # ties (even / odd lower neighbour), -0, smallest normal
        src = hip.DeviceBuffer.from_array(W)
        cnt = L.hpa_frag_bf16_elems(n, k)
        assert cnt == n * k
        dst = hip.DeviceBuffer(cnt * 2)
        hip.check(L.hpa_pack_frag_bf16(src.ptr, n, k, k, dst.ptr), "pack bf16")
        hip.check(L.hpa_synchronize())
        got = hip.from_frag_bf16(dst.download(cnt, np.uint16), n, k)
        assert np.array_equal(got, hip.to_bf16_bits(W))
        assert list(got[0, :4]) == [0x4080, 0x4082, 0x8000, 0x0080]


def test_pool_index_of_the_checker_is_the_librarys(hip):
    """chain_ref64.kv_index against hpa_pool_k_index / hpa_pool_v_index"""
    L = hip.lib()
    for P, bf16 in ((8, True), (64, False)):
        pool = hip.Pool(3, 12, P, 5, dtype=hip.HPA_BF16 if bf16 else hip.HPA_F32)
        geom = cr.pool_geom(3, 5, P, bf16)
        for layer, page, slot in ((0, 0, 0), (1, 3, P - 1), (2, 4, 5)):
            ki, vi = cr.kv_index(geom, layer, page, slot)
            for c in (0, 3, 4, 9, 63, 64, 700, 767):
                assert ki[c] == L.hpa_pool_k_index(pool.ref, layer, page, c // 64, slot, c % 64)
                assert vi[c] == L.hpa_pool_v_index(pool.ref, layer, page, c // 64, slot, c % 64)
        pool.destroy()


@pytest.mark.parametrize("B,P,pool_t,last", CHAIN_CASES, ids=[f"B{b}-P{p}-{t}-last{l}" for b, p, t, l in CHAIN_CASES])
def test_chain_phases_against_float64(hip, weights, B, P, pool_t, last):
    inp, pg, geom, out = _launch(hip, weights, B, P, pool_t, last)
    ratios, failures = cr.check_launch(inp, pg, geom, out, last=last, collect=True)
    print(_line(f"B={B} P={P} {pool_t} last={last}", ratios), failures or "")
    assert not failures, failures
    assert out["err_sticky"] == 0
    assert set(ratios) >= ({"B", "C", "D", "stats"} if last else {"B", "C", "D", "E"})
    # the inputs are off the synthetic regime: from the float64 side alone
    res2 = hip.from_frag(out["res2"], B, C).astype(np.float64)
    res = hip.from_frag(out["res"], B, C).astype(np.float64)
    cr.input_conditions(res2, inp["ln2_w"], inp["ln2_b"], "res2 (LN2)")
    cr.input_conditions(res, inp["ln1_w"], inp["ln1_b"], "res (LN1)")


@pytest.mark.parametrize("B,P,pool_t", FIRST_CASES, ids=[f"B{b}-P{p}-{t}" for b, p, t in FIRST_CASES])
def test_first_launch_against_float64(hip, weights, B, P, pool_t):
    inp, pg, geom, out = _launch(hip, weights, B, P, pool_t, first=True)
    assert inp["tokens"].min() == 0 and (B == 1 or inp["tokens"].max() == inp["V"] - 1)
    assert (B == 1 or pg["pos"].min() == 0) and pg["pos"].max() == len(inp["wpe"]) - 1
    ratios, failures = cr.check_launch(inp, pg, geom, out, first=True, layer=-1, collect=True)
    print(_line(f"first B={B} P={P} {pool_t}", ratios), failures or "")
    assert not failures, failures
    assert "E" in ratios
    cr.input_conditions(hip.from_frag(out["res"], B, C).astype(np.float64), inp["ln1_w"], inp["ln1_b"], "embedding")


_BITWISE = ("res2", "fch", "res", "q", "slab", "ctr", "pool_after")


def test_chain_is_repeatable(hip, weights):
    """the same case launched twice, counters zero both times: every output
    buffer, the slab and the pool bit-identical"""
    one = _launch(hip, weights, 40, 8, "bf16")[3]
    two = _launch(hip, weights, 40, 8, "bf16", cache=False)[3]
    for name in _BITWISE:
        assert np.array_equal(np.asarray(one[name]).view(np.uint8), np.asarray(two[name]).view(np.uint8)), name


def test_rows_do_not_depend_on_the_batch(hip, weights):
    """rows 0..39 at B = 40 against the same rows, same inputs, inside B = 200 (13
    row blocks against 3: other workgroups, row groups and quads): res2, fch, res,
    q_out and the K/V rows bit for bit -- "a row's summation order depends on
    nothing but the phase" (hpa_chain_b16.hip)"""
    small = _launch(hip, weights, 40, 8, "bf16")
    big = _launch(hip, weights, 200, 8, "bf16", cache=False)
    n = 40
    assert np.array_equal(small[0]["res"][:n], big[0]["res"][:n]) and np.array_equal(small[0]["att"][:n], big[0]["att"][:n])
    for name in ("res2", "res"):
        x, y = hip.from_frag(small[3][name], n, C), hip.from_frag(big[3][name], n, C)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    assert np.array_equal(hip.from_frag_bf16(small[3]["fch"], n, 4 * C), hip.from_frag_bf16(big[3]["fch"], n, 4 * C))
    assert np.array_equal(small[3]["q"][:n].view(np.uint32), big[3]["q"][:n].view(np.uint32))
    rows = []
    for inp, pg, geom, out in (small, big):
        assert not cr.check_launch(inp, pg, geom, out, collect=True)[1]
        pos = pg["pos"][:n].astype(np.int64)
        ki, vi = cr.kv_index(geom, 1, pg["bt"][np.arange(n), pos // 8], pos % 8)
        rows.append((out["pool_after"][ki], out["pool_after"][vi]))
    assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1])
