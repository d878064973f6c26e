"""The MXFP8 activation rule's numpy mirror (pagedattn.quantize_mxfp8_rows) at its edges.  CPU only."""
import numpy as np

import pagedattn as pa


def _group(vals):
    g = np.zeros((1, 32), np.float32)
    g[0, :len(vals)] = vals
    return pa.quantize_mxfp8_rows(g)


def test_scale_rule_edges():
    up = np.nextafter(np.float32(448), np.float32(1e9))
    for t in (-20, 0, 7):
        c, s_, _ = _group([np.ldexp(448.0, t)])
        assert s_[0, 0] == 127 + t and c[0, 0] == 0x7E  # amax = 448 2^t: x = 448, the largest code
        assert _group([np.ldexp(up, t)])[1][0, 0] == 128 + t     # the next float: one exponent up
        assert _group([np.ldexp(np.float32(0.875), t)])[1][0, 0] == 127 + t - 9   # m = 0.875 stays at e - 9
        assert _group([np.ldexp(np.nextafter(np.float32(0.875), np.float32(1)), t)])[1][0, 0] == 127 + t - 8
    assert _group([])[1][0, 0] == 127 and not _group([])[0].any()                  # a zero group: t = 0, code 0
    c, s, _ = _group([2.0 ** 100, 1.0])                                            # t clamped: the code saturates
    assert s[0, 0] == 127 + 64 and c[0, 0] == 0x7E and c[0, 1] == 0 and _group([2.0 ** -100])[1][0, 0] == 127 - 64


def test_ties_to_even_and_subnormals():
    # amax 448 (t = 0).  17, 19: ties between 16 / 18 / 20 go to the even mantissa; 2^-9 units below 2^-6
    c, _, d = _group([448, 17, 19, -17, 1.5 * 2 ** -9, 2.5 * 2 ** -9, 0.5 * 2 ** -9, 0.51 * 2 ** -9, 7.5 * 2 ** -9, -2.0 ** -9])
    assert c[0, :10].tolist() == [0x7E, 0x58, 0x5A, 0xD8, 2, 2, 0, 1, 8, 0x81]
    assert d[0, :10].tolist() == [448, 16, 20, -16, 2 ** -8, 2 ** -8, 0, 2 ** -9, 2 ** -6, -2.0 ** -9]


def test_error_at_most_half_a_step():
    rng = np.random.default_rng(0)
    A = (rng.standard_normal((64, 256)) * np.exp2(rng.integers(-30, 11, (64, 8)).repeat(32, 1))).astype(np.float32)
    c, s, d = pa.quantize_mxfp8_rows(A)
    y = np.abs(A.astype(np.float64)) * np.exp2(127.0 - s.repeat(32, 1))
    step = np.exp2(np.maximum(np.floor(np.log2(np.maximum(y, 2.0 ** -9))), -6) - 3)   # e4m3 spacing at y
    assert y.max() <= 448 and np.all(np.abs(d - A) <= 0.5 * step * np.exp2(s.repeat(32, 1) - 127.0))
    assert np.array_equal(pa.from_fp8_bits(c).astype(np.float64) * np.exp2(s.repeat(32, 1) - 127.0), d)
