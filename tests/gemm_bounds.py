"""The fused GEMM's float64 references and error bounds, shared by
tests/test_gpu_fused.py (the kernels one by one) and tests/dense_ref64.py (the
LNf / logits tail of the dense pass).  Numpy only.

fp32 weights:  |gpu - a @ W.T| <= 4e-6 * sum_k |a||w| + 2e-6  (fp32 MFMA chains).
bf16 weights:  the reference is the float64 product of the bf16-rounded
operands; an A element whose float64 value sits within 1e-5 relative of a bf16
rounding midpoint may round either way on the GPU (its LayerNorm is fp32), which
is one bf16 ulp (2^-7 |a| bound) there, added to the fp32 bound.
"""
import numpy as np


def rbf16(x):
    """fp32 -> bf16 value (round to nearest even, finite inputs), as fp32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_ambiguous(a64):
    """elements within 1e-5 relative of a bf16 rounding midpoint"""
    a32 = a64.astype(np.float32)
    lo = a32.view(np.uint32) & np.uint32(0xFFFF0000)
    mid = (lo | np.uint32(0x8000)).view(np.float32).astype(np.float64)
    return np.abs(a64 - mid) <= 1e-5 * np.abs(a64)


def fp32_bound(a, W):
    """4e-6 * sum_k |a||w| + 2e-6 for a (M, K) and W (N, K), float64"""
    return 4e-6 * (np.abs(a) @ np.abs(np.asarray(W, np.float64)).T) + 2e-6


def bf16_operands(a, W):
    """a (M, K) float64 and W (N, K) fp32 -> (a, W, extra): both rounded to bf16
    (a through fp32), as float64, and the ambiguous-midpoint term of the bound"""
    amb = bf16_ambiguous(a)
    ab = rbf16(a.astype(np.float32)).astype(np.float64)
    Wb = rbf16(W).astype(np.float64)
    extra = (amb * np.abs(a) * 2.0 ** -7) @ np.abs(Wb).T
    return ab, Wb, extra


def product_and_bound(a, W, w_bf16):
    """(a @ W.T, bound) of the numeric mode: the reference and the bound the
    fused GEMM's tests hold a LOGITS-style product to (no bias)"""
    a = np.asarray(a, np.float64)
    extra = 0.0
    if w_bf16:
        a, W, extra = bf16_operands(a, np.asarray(W, np.float32))
    W = np.asarray(W, np.float64)
    return a @ W.T, fp32_bound(a, W) + extra
