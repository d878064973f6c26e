"""The numpy mirror of the MXFP4 weight quantiser (pagedattn.quantize_mxfp4_rows:
hpa_pack_frag_fp4's rule restated) on hand-built groups.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm.c-paged_amd"))
import pagedattn as pa  # noqa: E402


def _group(absmax, fill=0.0):
    g = np.full(32, fill, np.float32)
    g[7] = absmax
    return g


@pytest.mark.parametrize("e", [-20, 0, 9])
def test_scale_from_absmax(e):
    """absmax 6 * 2^e: t = e, code 7; one ulp above: t = e + 1; m = 0.75 exactly (3 * 2^e): t = e - 1"""
    above = np.nextafter(np.float32(6 * 2.0 ** e), np.float32(np.inf))
    W = np.stack([_group(6 * 2.0 ** e), _group(-above), _group(3 * 2.0 ** e)]).reshape(1, 96)
    codes, sb, Wd = pa.quantize_mxfp4_rows(W)
    assert sb.tolist() == [[127 + e, 127 + e + 1, 127 + e - 1]]
    assert codes[0, [7, 39, 71]].tolist() == [7, 8 | 5, 7]  # 6 | -(3 * 2) | 6 at half the scale
    assert Wd[0, [7, 39, 71]].tolist() == [6 * 2.0 ** e, -6 * 2.0 ** e, 3 * 2.0 ** e]


def test_zero_group_and_exponent_clamp():
    W = np.stack([_group(0), _group(2.0 ** -100), _group(-2.0 ** 100), _group(1.0)]).reshape(2, 64)
    codes, sb, Wd = pa.quantize_mxfp4_rows(W)
    assert sb.tolist() == [[127, 127 - 64], [127 + 64, 127 - 2]]
    assert np.all(codes[0] == 0) and np.all(Wd[0] == 0)  # 2^-100 * 2^64 rounds to code 0
    assert codes[1, 7] == 8 | 7 and Wd[1, 7] == -6 * 2.0 ** 64  # saturates


@pytest.mark.parametrize("sign", [1, -1])
def test_ties_go_to_the_even_mantissa(sign):
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)
    W = _group(6.0)  # t = 0
    W[8:15] = sign * ties
    W[16:23] = sign * np.nextafter(ties, np.float32(0))   # just below each tie: the lower code
    W[24:31] = sign * np.nextafter(ties, np.float32(8))   # just above: the upper code
    codes, sb, Wd = pa.quantize_mxfp4_rows(np.tile(W, 2)[None])
    s = 8 if sign < 0 else 0
    assert sb[0, 0] == 127
    assert codes[0, 8:15].tolist() == [s | c for c in (0, 2, 2, 4, 4, 6, 6)]
    assert Wd[0, 8:15].tolist() == [sign * v for v in (0, 1, 1, 2, 2, 4, 4)]
    assert codes[0, 16:23].tolist() == [s | c for c in range(7)]
    assert codes[0, 24:31].tolist() == [s | c for c in range(1, 8)]


def test_dequantised_values_are_bf16_and_within_half_a_step():
    rng = np.random.default_rng(11)
    W = rng.standard_normal((41, 128)).astype(np.float32) * np.exp2(rng.integers(-30, 11, (41, 4))).repeat(32, 1).astype(np.float32)
    codes, sb, Wd = pa.quantize_mxfp4_rows(W)
    assert codes.shape == W.shape and codes.max() < 16 and sb.shape == (41, 4)
    assert np.array_equal(pa.round_bf16(Wd).view(np.uint32), Wd.view(np.uint32))
    t = sb.astype(np.int32).repeat(32, 1) - 127
    assert np.all(np.abs(W.astype(np.float64) - Wd) <= np.exp2(t))  # half the widest code spacing (4 -> 6)
    r = np.abs(W).reshape(41, 4, 32).max(2) / np.exp2(sb.astype(np.int32) - 127)
    assert np.all((r > 3) & (r <= 6))
    assert np.array_equal(np.where(codes & 8, -1, 1) * pa.E2M1[codes & 7] * np.exp2(t).astype(np.float32), Wd)
