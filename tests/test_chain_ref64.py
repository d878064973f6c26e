"""CPU self-test of tests/chain_ref64.py: a numpy emulation of the bf16 chain
(fp32 one-pass LayerNorm, round-to-nearest-even operands, float64 products
rounded to fp32, page writes into a host image, the counter arrivals walked
workgroup by workgroup as the kernel deals its units) must pass every check
with every ratio below 0.5 (phase C below 1: see there), and every mutant of it must be rejected by the
check named for it.  No GPU, no library call.
"""
import math

import numpy as np
import pytest

import chain_ref64 as cr
from pagedattn import frag_bf16_index, from_bf16_bits, from_frag_bf16, to_frag

C = cr.C
f32 = np.float32


def _bits(x, mode="rne"):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    if mode == "rne":
        u = u + 0x7FFF + ((u >> 16) & 1)
    elif mode == "away":  # ties away from zero
        u = u + 0x8000
    else:
        assert mode == "trunc"
    return (u >> 16).astype(np.uint16)


def _gemm(a, W, drop=None):
    a = np.array(a, np.float64)
    if drop is not None:
        a[:, 32 * drop:32 * drop + 32] = 0
    return (a @ W.T).astype(np.float32)


def _ln32(x, g, b, eps):
    """the kernel's LayerNorm in fp32: one-pass statistics, (rs * (x - m)) * g + b"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):  # the eps = 0 mutant divides by zero on the padded rows
        return _ln32_(x, g, b, eps)


def _ln32_(x, g, b, eps):
    s1 = x.sum(-1, dtype=np.float32, keepdims=True)
    s2 = (x * x).sum(-1, dtype=np.float32, keepdims=True)
    m = s1 / f32(C)
    var = np.maximum(s2 / f32(C) - m * m, f32(0))
    rs = f32(1) / np.sqrt(var + f32(eps), dtype=np.float32)
    return (rs * (x - m)) * g + b


def _gelu32(x, erf=False):
    x = x.astype(np.float64)
    if erf:
        return (0.5 * x * (1 + np.vectorize(math.erf)(x / math.sqrt(2)))).astype(np.float32)
    return cr.gelu(x).astype(np.float32)


def _counters(B, miss=None):
    """the arrivals of hpa_chain_b16.hip, workgroup by workgroup"""
    c = np.zeros(cr.K_LINES * cr.K_PAD, np.int32)
    R = (B + 15) // 16
    RH, RQ = (R + 1) // 2, (R + 3) // 4

    def arrive(line):
        c[line * cr.K_PAD] += 1
    for bid in range(256):
        if bid < R * 16:
            arrive(cr.K_X1 + bid // 16)
        if bid < RH * 32:
            g, rb0 = bid % 32, 2 * (bid // 32)
            p = g * 6 // 48
            arrive(cr.K_H + rb0 * 4 + p)
            if rb0 + 1 < R:
                arrive(cr.K_H + (rb0 + 1) * 4 + p)
        if bid < RQ * 64:
            g, rg = bid % 16, bid // 64
            arrive(cr.K_TICK + rg * 16 + g)
            if c[(cr.K_TICK + rg * 16 + g) * cr.K_PAD] == 4:
                for r in range(4):
                    if 4 * rg + r < R:
                        arrive(cr.K_X2 + 4 * rg + r)
    if miss is not None:
        c[miss * cr.K_PAD] -= 1
    return c


def emulate(inp, pg, geom, last=0, first=False, layer=0, mut=()):
    """one launch.  mut: names of the deviations to apply"""
    B, Mp, W = inp["B"], inp["Mp"], inp["W64"]
    mode = "trunc" if "trunc" in mut else "away" if "away" in mut else "rne"
    eps = 1e-6 if "eps1e-6" in mut else 0.0 if "eps0" in mut else 1e-5
    rb = lambda x: from_bf16_bits(_bits(x, mode)).astype(np.float64)
    live = np.arange(Mp)[:, None] < B
    out = dict(err=0, stats=None, guards={})
    n_el = geom["L"] * geom["layer_elems"]
    pool = np.full(n_el, 0xFFFF if geom["bf16"] else 0xFFFFFFFF, np.uint16 if geom["bf16"] else np.uint32)
    out["pool_before"] = pool.copy()
    q = np.full((Mp, C), cr.SENT32, np.uint32).view(np.float32)
    pos = pg["pos"]
    if first:
        res = np.zeros((Mp, C), np.float32)
        res[:B] = inp["wte"][inp["tokens"]] + inp["wpe"][pos]
        out["zero"] = np.concatenate([np.zeros(64, np.uint32), np.full(16, 0xFFFFFFFF, np.uint32)])
        out["zero_words"] = 64
        if "embed" in mut:
            res[B - 1, 17] = np.nextafter(res[B - 1, 17], f32(9))
    else:
        res2 = inp["res"] + (_gemm(rb(inp["att"]), W["w_ap"], 3 if "dropB" in mut else None) + inp["b_ap"])
        res2 = np.where(live, res2, f32(0)).astype(np.float32)
        if "padded" in mut:
            res2[Mp - 1, 100] = f32(1e-3)
        a = rb(_ln32(res2, inp["ln2_w"], inp["ln2_b"], eps))
        pre = _gemm(a, W["w_fc"], 11 if "dropC" in mut else None) + inp["b_fc"]
        h = np.where(live, _gelu32(pre, erf="erf" in mut), f32(0)).astype(np.float32)
        m, k = np.meshgrid(np.arange(Mp), np.arange(4 * C), indexing="ij")
        kk = k.copy()
        if "lanegroup" in mut:  # 32-deep step 5 of row block 0: lane group 1 stored at group 2's offset and back
            sel = (m < 16) & (k >> 5 == 5)
            grp = (k >> 2) & 3
            kk = np.where(sel & (grp == 1), k + 4, np.where(sel & (grp == 2), k - 4, k))
        fch = np.zeros(Mp * 4 * C, np.uint16)
        fch[frag_bf16_index(m, kk, 4 * C)] = _bits(h)
        hv = from_bf16_bits(from_frag_bf16(fch, Mp, 4 * C)).astype(np.float64)
        parts = []
        for p in range(4):
            ap = np.zeros_like(hv)
            ap[:, p * C:(p + 1) * C] = hv[:, p * C:(p + 1) * C]
            parts.append(_gemm(ap, W["w_fp"], 24 * p + 7 if ("dropD" in mut and p == 2) else None))
        if "part_dropped" in mut:
            parts[2] = np.zeros_like(parts[2])
        if "part_twice" in mut:
            parts[3] = parts[1]
        tot = ((parts[0] + parts[1]) + parts[2]) + parts[3] + inp["b_fp"]
        res = np.where(live, res2 + tot, f32(0)).astype(np.float32)
        out["res2"], out["fch"] = to_frag(res2), fch
        out["ctr"] = _counters(B, cr.K_X1 + 1 if "arrival" in mut else None)
        if last:
            smp = Mp + 16
            st = np.full((C // 16, smp, 2), cr.SENT32, np.uint32).view(np.float32)
            t = res.reshape(Mp, C // 16, 16).transpose(1, 0, 2)
            st[:, :Mp, 0] = t.sum(-1, dtype=np.float32)
            st[:, :Mp, 1] = (t * t).sum(-1, dtype=np.float32)
            out["stats"], out["stats_mp"] = st.ravel(), smp
    out["res"] = to_frag(res)
    if not last:
        a = rb(_ln32(res, inp["ln1_w"], inp["ln1_b"], eps))
        if "ulp" in mut:  # one operand element a single bf16 ulp off
            one = _bits(np.array([a[B // 2, 300]], np.float32))
            a[B // 2, 300] = from_bf16_bits(one + np.uint16(1))[0]
        y = _gemm(a, W["w_qkv"], 20 if "dropE" in mut else None) + inp["b_qkv"]
        q[:B] = y[:B, :C]
        wpos = pos.copy()
        if "swap_pos" in mut:
            wpos[[1, 2]] = wpos[[2, 1]]
        P = geom["P"]
        page = pg["bt"][np.arange(B), wpos // P].copy()
        if "free_page" in mut:
            page[B - 1] = pg["free_pages"][3]
        ok = page >= 0
        ki, vi = cr.kv_index(geom, layer + 1, page[ok], wpos[ok] % P)
        store = (lambda x: _bits(x)) if geom["bf16"] else (lambda x: x.view(np.uint32))
        pool[ki] = store(np.ascontiguousarray(y[:B, C:2 * C][ok]))
        pool[vi] = store(np.ascontiguousarray(y[:B, 2 * C:][ok]))
    out["q"], out["pool_after"] = q, pool
    return out


B, P = 40, 8


@pytest.fixture(scope="module")
def case():
    inp = cr.make_inputs(B, seed=5)
    pg = cr.make_paging(B, P)
    inp["wpe"] = inp["wpe"][:int(pg["pos"].max()) + 1]
    return inp, pg


def _geom(pg, bf16):
    return cr.pool_geom(3, pg["pages"], pg["P"], bf16)


@pytest.fixture(scope="module")
def clean(case):
    """the unmodified emulation's launch on a bf16 pool, checked once"""
    inp, pg = case
    geom = _geom(pg, True)
    out = emulate(inp, pg, geom)
    return out, cr.check_launch(inp, pg, geom, out)


def test_inputs_are_off_the_synthetic_regime(case, clean):
    """on float64 values alone: LN2's input and LN1's (chain and first launch)"""
    inp, pg = case
    out = clean[0]
    from pagedattn import from_frag
    cr.input_conditions(from_frag(out["res2"], B, C), inp["ln2_w"], inp["ln2_b"], "res2")
    cr.input_conditions(from_frag(out["res"], B, C), inp["ln1_w"], inp["ln1_b"], "res")
    cr.input_conditions(inp["wte"][inp["tokens"]].astype(np.float64) + inp["wpe"][pg["pos"]], inp["ln1_w"],
                        inp["ln1_b"], "embedding")
    assert inp["tokens"].min() == 0 and inp["tokens"].max() == inp["V"] - 1
    assert pg["pos"].min() == 0 and pg["pos"].max() == len(inp["wpe"]) - 1


def test_att_carries_the_rounding_edges(case):
    """ties with an even and an odd lower neighbour, their fp32 neighbours, +-0 and
    the smallest normal, where round-to-nearest-even, truncation and ties-away differ"""
    att = case[0]["att"]
    for r in range(0, B, 16):
        row = att[r]
        rne, tr, aw = _bits(row), _bits(row, "trunc"), _bits(row, "away")
        assert (rne[[5, 402]] == 0x4080).all() and (aw[[5, 402]] == 0x4081).all()      # even: down / away up
        assert (rne[[201, 470]] == 0x4082).all() and (tr[[201, 470]] == 0x4081).all()  # odd: up / truncated down
        assert rne[600] == 0x4080 and rne[611] == 0x4081 and rne[650] == 0xC081 and rne[661] == 0xC082
        assert rne[700] == 0 and rne[701] == 0x8000 and rne[766] == 0x0080 and rne[767] == 0x8080


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("last", [0, 1])
def test_emulation_passes_every_check(case, clean, bf16, last):
    inp, pg = case
    if bf16 and not last:
        ratios = clean[1][0]
    else:
        geom = _geom(pg, bf16)
        ratios, _ = cr.check_launch(inp, pg, geom, emulate(inp, pg, geom, last=last), last=last)
    print("CHAINREF", "bf16" if bf16 else "f32", "last" if last else "", ratios)
    want = {"B", "C", "D", "S2"} | ({"stats"} if last else {"E", "S1"})
    assert set(ratios) == want
    for name in want - {"S1", "S2", "C"}:
        assert ratios[name] < 0.5, (name, ratios[name])
    # C's allowance is centred on rb_lo: an operand that legally rounds to rb_hi in all of S
    # spends up to the whole flip, so a correct chain can come near 1 there (0.77 here)
    assert ratios["C"] < 1.0, ratios["C"]
    assert max(ratios.get("S1", 0), ratios["S2"]) <= 32


@pytest.mark.parametrize("bf16", [True, False])
def test_first_launch_emulation_passes(case, bf16):
    inp, pg = case
    geom = _geom(pg, bf16)
    ratios, _ = cr.check_launch(inp, pg, geom, emulate(inp, pg, geom, first=True, layer=-1), first=True, layer=-1)
    assert set(ratios) == {"E", "S1"} and ratios["E"] < 0.5, ratios


MUTANTS = [
    ("trunc", {"B", "E"}), ("away", {"B"}), ("eps1e-6", {"C", "E"}), ("eps0", {"C", "E"}),
    ("dropB", {"B"}), ("dropC", {"C"}), ("dropD", {"D"}), ("dropE", {"E"}),
    ("part_dropped", {"D"}), ("part_twice", {"D"}), ("erf", {"C"}), ("lanegroup", {"C"}),
    ("swap_pos", {"placement"}), ("free_page", {"placement"}), ("padded", {"padded"}),
    ("arrival", {"protocol"}), ("ulp", {"E"}),
]


@pytest.mark.parametrize("mut,must_fail", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_mutant_is_rejected_by_its_check(case, mut, must_fail):
    """each phase is checked on the emulation's own input to it, so a mutant fails
    the checks of the phases it touches and no other"""
    inp, pg = case
    geom = _geom(pg, True)
    out = emulate(inp, pg, geom, mut={mut})
    _, failures = cr.check_launch(inp, pg, geom, out, collect=True)
    assert must_fail <= set(failures), (mut, failures)
    allowed = must_fail | {"trunc": {"C"}, "away": {"C", "E"}, "padded": {"C"}}.get(mut, set())
    assert set(failures) <= allowed, (mut, failures)
    with pytest.raises(cr.ChainMismatch):
        cr.check_launch(inp, pg, geom, out)


def test_truncation_and_one_ulp_fail_phase_e_by_a_wide_margin(case):
    """the resolved rounding forgives a legal rounding only: a truncated operand
    and a single element one bf16 ulp off miss the bound many times over"""
    inp, pg = case
    geom = _geom(pg, False)
    for mut, margin in (("trunc", 50), ("ulp", 2)):
        out = emulate(inp, pg, geom, mut={mut})
        with pytest.raises(cr.ChainMismatch) as e:
            cr.check_qkv(*_qkv_args(inp, pg, geom, out))
        assert e.value.check == "E"
        worst = float(str(e.value).rsplit("worst ", 1)[1])
        assert worst > margin, (mut, worst)


def _qkv_args(inp, pg, geom, out):
    from pagedattn import from_frag
    k, v = cr.check_placement(geom, out["pool_before"], out["pool_after"], 1, pg["bt"], pg["pos"], B)
    return (from_frag(out["res"], inp["Mp"], C), inp["ln1_w"], inp["ln1_b"], inp["W64"]["w_qkv"], inp["b_qkv"],
            out["q"], k, v, geom["bf16"], B)


def test_first_launch_mutants(case):
    inp, pg = case
    geom = _geom(pg, True)
    out = emulate(inp, pg, geom, first=True, layer=-1, mut={"embed"})
    assert "embed" in cr.check_launch(inp, pg, geom, out, first=True, layer=-1, collect=True)[1]
    out = emulate(inp, pg, geom, first=True, layer=-1)
    out["zero"][64] = 0  # one word past zero_bytes zeroed
    assert "guard" in cr.check_launch(inp, pg, geom, out, first=True, layer=-1, collect=True)[1]
    out = emulate(inp, pg, geom, first=True, layer=-1)
    out["zero"][63] = 7
    assert "protocol" in cr.check_launch(inp, pg, geom, out, first=True, layer=-1, collect=True)[1]


def test_guards_and_stray_writes_are_seen(case):
    inp, pg = case
    geom = _geom(pg, True)
    out = emulate(inp, pg, geom)
    out["q"][B, 3] = 0.0  # a q_out row the batch does not have
    assert "guard" in cr.check_launch(inp, pg, geom, out, collect=True)[1]
    out = emulate(inp, pg, geom, last=1)
    out["pool_after"][5] = 0  # a launch without a qkv phase wrote the pool
    assert "placement" in cr.check_launch(inp, pg, geom, out, last=1, collect=True)[1]
    out = emulate(inp, pg, geom, last=1)
    out["stats"][0] *= f32(1.001)
    assert "stats" in cr.check_launch(inp, pg, geom, out, last=1, collect=True)[1]
    out = emulate(inp, pg, geom)
    out["ctr"][3] = 1  # an int of a counter line that is no counter
    assert "protocol" in cr.check_launch(inp, pg, geom, out, collect=True)[1]
    out = emulate(inp, pg, geom)
    out["err"] = 3
    assert "protocol" in cr.check_launch(inp, pg, geom, out, collect=True)[1]


def test_expected_counters_follow_the_kernels_arrivals():
    """the closed form of the checker against the workgroup-by-workgroup walk"""
    for b in (1, 16, 17, 40, 72, 200, 256):
        assert np.array_equal(cr.expected_counters(b), _counters(b)), b
    R = 3
    c = cr.expected_counters(40)
    assert c[(cr.K_X1 + R - 1) * cr.K_PAD] == 16 and c[(cr.K_X1 + R) * cr.K_PAD] == 0
    assert c[(cr.K_H + 4 * (R - 1) + 3) * cr.K_PAD] == 8 and c[cr.K_TICK * cr.K_PAD] == 4
    assert c[(cr.K_TICK + 16) * cr.K_PAD] == 0  # one quad only
