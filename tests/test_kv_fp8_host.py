"""The fp8 (OCP e4m3fn) KV pool's host side, no GPU: the numpy codec of
pagedattn against first principles and against torch.float8_e4m3fn, the
layout helpers of an HPA_FP8 pool, and the HpaKVPool struct mirror.

The stored value (include/hip_paged_attn.h): code = e4m3fn_rne(clamp(x * inv,
-448, 448)), value = decode(code) * scale.  e4m3fn: 1 sign, 4 exponent bits
(bias 7), 3 mantissa bits, no infinities, NaN = 0x7f / 0xff, subnormals
m * 2^-9, largest finite value 448.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pagedattn as pa

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _value(code):
    """the value of a code from its sign, exponent and mantissa fields (exact in float64)"""
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return float("nan")
    mag = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -mag if s else mag


FINITE = [c for c in range(256) if (c & 0x7F) != 0x7F]          # 254 codes
POS = sorted((_value(c), c) for c in FINITE if c < 0x80)        # 127 values 0 .. 448 with their codes


def _brute(x):
    """nearest of the 254 finite values to x (float64 arithmetic: the values and
    the fp32 inputs are exact there), ties to the even code, saturating; the
    sign of x is kept (so -0.0 and negative underflows give 0x80)"""
    out = np.empty(len(x), np.uint8)
    vals = np.array([v for v, _ in POS])
    codes = np.array([c for _, c in POS])
    for i, xi in enumerate(np.asarray(x, np.float64)):
        a = min(abs(xi), 448.0)
        d = np.abs(vals - a)
        best = np.nonzero(d == d.min())[0]
        c = codes[best[0]] if len(best) == 1 else [c for c in codes[best] if c % 2 == 0][0]
        out[i] = c | (0x80 if np.signbit(xi) else 0)
    return out


def _inputs():
    rng = np.random.default_rng(448)
    vals = np.array([v for v, _ in POS], np.float64)
    mids = (vals[1:] + vals[:-1]) / 2  # 9 significant bits at most: exact in fp32
    assert np.array_equal(mids.astype(np.float32).astype(np.float64), mids)
    rand = np.exp2(rng.uniform(-12, 10, 10000)) * rng.choice([-1.0, 1.0], 10000)
    tiny = [2.0 ** -10 * 0.999, 2.0 ** -11, 2.0 ** -12, 1e-6, 2.0 ** -30, 1e-45]
    x = np.concatenate([mids, -mids, vals, -vals, [0.0, -0.0], [448.0, -448.0, 449.0, -449.0, 1e4, -1e4],
                        tiny, [-t for t in tiny], rand])
    return x.astype(np.float32)


def test_from_fp8_bits_matches_the_bit_fields():
    got = pa.from_fp8_bits(np.arange(256, dtype=np.uint8))
    assert got.dtype == np.float32
    for c in range(256):
        want = _value(c)
        if want != want:
            assert np.isnan(got[c]), c
        else:
            assert got[c] == want and np.signbit(got[c]) == (c >= 0x80), (c, got[c], want)
    assert got[0x7E] == 448.0 and got[0x01] == 2.0 ** -9 and got[0x08] == 2.0 ** -6


def test_to_fp8_bits_is_nearest_even_with_saturation():
    x = _inputs()
    got = pa.to_fp8_bits(x)
    want = _brute(x)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # the named cases, spelled out
    f = lambda *v: list(pa.to_fp8_bits(np.array(v, np.float32)))
    assert f(448.0, -448.0, 449.0, -449.0, 1e4, -1e4) == [0x7E, 0xFE, 0x7E, 0xFE, 0x7E, 0xFE]
    assert f(0.0, -0.0, 2.0 ** -11, -2.0 ** -11, 2.0 ** -10) == [0x00, 0x80, 0x00, 0x80, 0x00]  # the tie at 2^-10 goes to even (0)
    assert f(1.5 * 2.0 ** -10, 2.0 ** -9) == [0x01, 0x01]
    assert f(float("nan"))[0] & 0x7F == 0x7F
    # every representable value round-trips
    codes = np.array(FINITE, np.uint8)
    assert np.array_equal(pa.to_fp8_bits(pa.from_fp8_bits(codes)), codes)


def test_round_fp8_applies_the_scale_in_fp32():
    x = np.array([0.3, -1.0, 500.0, 1e-4], np.float32)
    for scale in (1.0, 0.37, 2.0 ** -3, 64.0):
        s = np.float32(scale)
        inv = np.float32(1.0) / s
        want = pa.from_fp8_bits(pa.to_fp8_bits((x * inv).astype(np.float32))) * s
        assert np.array_equal(pa.round_fp8(x, scale), want.astype(np.float32))
    assert pa.round_fp8(np.float32(500.0), 1.0) == 448.0
    # per-head broadcast
    got = pa.round_fp8(np.ones((2, 3), np.float32) * 0.3, np.array([1.0, 0.37, 0.125], np.float32))
    assert got.shape == (2, 3) and got[0, 1] == pa.round_fp8(np.float32(0.3), 0.37)


def test_codec_matches_torch_float8_e4m3fn(tmp_path):
    """the same inputs through torch, in a fresh child process that never touches a GPU"""
    x = _inputs()
    np.save(tmp_path / "x.npy", x)
    script = ("import sys, numpy as np, torch\n"
              "x = torch.from_numpy(np.load(sys.argv[1]))\n"
              "b = x.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()\n"
              "np.save(sys.argv[2], b)\n"
              "c = torch.arange(256, dtype=torch.int32).to(torch.uint8)\n"
              "np.save(sys.argv[3], c.view(torch.float8_e4m3fn).to(torch.float32).numpy())\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "x.npy"), str(tmp_path / "b.npy"),
                        str(tmp_path / "v.npy")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pa.to_fp8_bits(x), np.load(tmp_path / "b.npy"))
    v, mine = np.load(tmp_path / "v.npy"), pa.from_fp8_bits(np.arange(256, dtype=np.uint8))
    assert np.array_equal(np.isnan(v), np.isnan(mine))
    assert np.array_equal(v[~np.isnan(v)].view(np.uint32), mine[~np.isnan(mine)].view(np.uint32))


def _host_pool(P=16, NH=2, L=2, pages=5):
    s = pa.HpaKVPool()
    s.base = 0x100000
    s.num_layers, s.num_heads, s.head_size, s.page_size, s.num_pages = L, NH, 64, P, pages
    s.dtype = pa.HPA_FP8
    s.elem_bytes = 1
    s.page_elems = 2 * NH * P * 64
    s.layer_elems = pages * s.page_elems
    s.bytes = L * s.layer_elems
    return s


def test_fp8_pool_index_helpers_follow_the_documented_layout():
    """K tile [head_size/16][page_size][16], V tile [page_size][64], one byte per
    element; hpa_pool_tile is host pointer arithmetic on the struct's fields"""
    assert pa.HPA_FP8 == 2
    L = pa.lib()
    P, NH = 16, 2
    s = _host_pool(P, NH)
    ref = ctypes.byref(s)
    tile = P * 64
    for layer, page in ((0, 0), (1, 3)):
        base = layer * s.layer_elems + page * s.page_elems
        for head in range(NH):
            assert L.hpa_pool_tile(ref, layer, page, 0, head) == s.base + base + head * tile
            assert L.hpa_pool_tile(ref, layer, page, 1, head) == s.base + base + (NH + head) * tile
            for slot in range(P):
                for d in range(64):
                    assert L.hpa_pool_k_index(ref, layer, page, head, slot, d) == \
                        base + head * tile + ((d >> 4) * P + slot) * 16 + (d & 15)
                    assert L.hpa_pool_v_index(ref, layer, page, head, slot, d) == \
                        base + (NH + head) * tile + slot * 64 + d


def test_struct_mirror_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_paged_attn.h"\n'
                   'int main(void) { printf("%zu %zu %d\\n", sizeof(HpaKVPool), offsetof(HpaKVPool, scales), '
                   '(int)HPA_FP8); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe],
                   check=True)
    size, off, fp8 = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(pa.HpaKVPool) == size
    assert pa.HpaKVPool.scales.offset == off
    assert pa.HpaKVPool._fields_[-1][0] == "scales"  # the last member
    assert fp8 == pa.HPA_FP8


def test_new_entry_points_are_declared_and_bound():
    """test_abi.py's export check covers what the headers declare; here: they are declared"""
    hdr = open(os.path.join(REPO, "include", "hip_paged_attn.h")).read()
    eng = open(os.path.join(REPO, "include", "paged_infer.h")).read()
    assert "hpa_pool_set_scales(" in hdr and "HPA_FP8 = 2" in hdr
    assert "gpt2_decode_set_kv_scales(" in eng and "gpt2_decode_kv_scales(" in eng
    L = pa.lib()
    for name in ("hpa_pool_set_scales", "gpt2_decode_set_kv_scales", "gpt2_decode_kv_scales"):
        assert getattr(L, name).argtypes is not None
    for name in ("set_kv_scales", "kv_scales"):
        assert callable(getattr(pa.Model, name))
    assert callable(pa.Pool.set_scales)
