"""float64 reference of hpa_top_logprobs (hpa_top.hip).

For a row x of fp32 logits:
  topk64(x, k)  (ids, lps): ids = the first k columns under the order
                "logit descending as an fp32 comparison (-0.0 and +0.0 tie),
                equal logits by ascending column" -- a stable argsort of -x,
                truncated; lps = x[ids] - score_ref64.lse64(x) in float64.
  topk_brute    the same ids by an O(V k) selection that restates the rule
                (tests/test_top_ref64.py pins the two against each other)

The kernel's bound on every log-probability is score_ref64.kernel_bound's:
4e-6 + 2^-22 * max(|lse64|, |x[id]|).
"""
import numpy as np

import score_ref64 as sr


def topk64(x, k):
    """x: (rows, V) or (V,); returns (ids int64, lps float64) of shape (..., k)"""
    x = np.asarray(x, np.float32)
    one = x.ndim == 1
    x2 = x[None] if one else x
    # -x keeps fp32 comparisons: -(+0.0) = -0.0 == +0.0 = -(-0.0); the stable sort keeps equal values by column
    ids = np.argsort(-x2, axis=-1, kind="stable")[:, :k]
    lps = np.take_along_axis(x2.astype(np.float64), ids, -1) - sr.lse64(x2)[:, None]
    return (ids[0], lps[0]) if one else (ids, lps)


def topk_brute(x, k):
    """k rounds over one row: the largest remaining value, the lowest column among equals"""
    x = np.asarray(x, np.float32)
    taken = np.zeros(len(x), bool)
    ids = []
    for _ in range(k):
        best = -1
        for i in range(len(x)):
            if taken[i]:
                continue
            if best < 0 or x[i] > x[best]:  # strict: an equal later column never replaces an earlier one
                best = i
        taken[best] = True
        ids.append(best)
    return np.array(ids, np.int64)


def bound(x, ids):
    """(rows, k) kernel bound at the columns ids of every row"""
    x = np.asarray(x, np.float64)
    picked = np.abs(np.take_along_axis(x, np.asarray(ids, np.int64), -1))
    return 4e-6 + 2.0 ** -22 * np.maximum(np.abs(sr.lse64(x))[:, None], picked)
