"""The numpy mirror of the fp8 weight quantiser (pagedattn.quantize_fp8_rows:
hpa_pack_frag_fp8's rule restated) and the layer plan under fp8 weights.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm.c-paged_amd"))
import pagedattn as pa  # noqa: E402


def _rows():
    rng = np.random.default_rng(7)
    ex = np.arange(-30, 11)
    W = rng.uniform(-1, 1, (len(ex) + 3, 128)).astype(np.float32)
    W[:len(ex)] *= np.exp2(ex)[:, None].astype(np.float32)
    W[-3] = 0                                  # a zero row
    W[-2] *= 0.5
    W[-2, 9] = 448 * 2.0 ** -5                 # absmax exactly 448 * 2^e
    W[-1, 1::2] *= 2.0 ** -9                   # elements below s * 2^-6: e4m3 subnormals
    return W


def test_quantize_fp8_rows():
    W = _rows()
    codes, s, Wd = pa.quantize_fp8_rows(W)
    absmax = np.abs(W).max(1)
    assert s[-3] == 1 and np.all(codes[-3] == 0)
    assert absmax[-2] / s[-2] == 448 and (codes[-2, 9] & 0x7F) == 0x7E
    sub = np.abs(W[-1]) < s[-1] * 2.0 ** -6
    assert sub.any() and np.all((codes[-1][sub] & 0x78) == 0)
    assert np.array_equal(pa.round_bf16(Wd).view(np.uint32), Wd.view(np.uint32))
    m, e = np.frexp(s)
    assert np.all(m == 0.5)  # powers of two
    live = absmax > 0
    r = absmax[live].astype(np.float64) / s[live]
    assert np.all((r > 224) & (r <= 448))
    W64, s64 = W.astype(np.float64), s.astype(np.float64)[:, None]
    assert np.all(np.abs(W64 - Wd) <= 2.0 ** -4 * np.abs(W64) + s64 * 2.0 ** -10)
    assert np.array_equal(pa.from_fp8_bits(codes) * s[:, None], Wd)


@pytest.mark.parametrize("C,NH", [(768, 12), (1600, 25)])
@pytest.mark.parametrize("B", [8, 64])
def test_layer_plan_fp8_weights_is_five_launches(C, NH, B):
    five = dict(form=0, chain=0, splits=1, first=0, attn_launch=0)
    for request in range(8):
        for kv in (pa.HPA_F32, pa.HPA_BF16, pa.HPA_FP8):
            assert pa.layer_plan(request, B, C, NH, 1024, kv_dtype=kv, w_bf16=2) == five
