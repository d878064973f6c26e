"""float64 reference of the scoring kernels (hpa_score.hip, HPA_FEPI_SCORE).

For a row x of fp32 logits, everything in float64:
  lse64(x)        the stable log-sum-exp: max + log(sum(exp(x - max)))
  logprob64(x, t) x[t] - lse64(x), the log-probability of column t
                  (t == -1: no target, 0.0)
  first_argmax(x) the lowest column holding the row's maximum

KERNEL_BOUND is the kernels' error bound against this reference on the SAME
fp32 logits (derivation: hpa_score.hip, DESIGN.md "Scoring"):
  |logprob - logprob64| <= 4e-6 + 2^-22 * max(|lse64|, |x[t]|)
"""
import numpy as np


def lse64(x):
    """log-sum-exp along the last axis, float64"""
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[..., 0]


def logprob64(x, targets):
    """x: (rows, V); targets: (rows,) columns, -1 = none (0.0)"""
    x = np.asarray(x, np.float64)
    t = np.asarray(targets, np.int64)
    picked = x[np.arange(x.shape[0]), np.where(t < 0, 0, t)]
    return np.where(t < 0, 0.0, picked - lse64(x))


def first_argmax(x):
    """lowest column of each row's maximum (numpy's argmax returns the first)"""
    return np.asarray(x).argmax(-1)


def kernel_bound(x, targets):
    """per-row bound of the kernels' log-probability against logprob64(x, targets)"""
    x = np.asarray(x, np.float64)
    t = np.asarray(targets, np.int64)
    picked = np.abs(x[np.arange(x.shape[0]), np.where(t < 0, 0, t)])
    return 4e-6 + 2.0 ** -22 * np.maximum(np.abs(lse64(x)), picked)
