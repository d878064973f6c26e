"""hpa_top_logprobs alone, on uploaded rows, against tests/top_ref64.py.

Shapes: V = 50257 with 8 rows (row stride V is odd, so the four 16-byte
alignments of a row's first column occur twice each), V = 33 and V = 20 (one
partial wave; k = 20 = V); k in {1, 5, 20}.

  ids        exactly the reference's (the order rule is the whole specification)
  top_lps, target_lp, lse   within score_ref64.kernel_bound of float64
  top_lps    non-increasing; a second launch identical bit for bit
  rows with active <= 0 and everything behind the last row keep the 0xFF fill

The bound is the project's scoring bound (derivation for this kernel's
summation order: the header of hpa_top.hip), not widened; measured worst on
the V = 50257 rows: 0.04 / 0.15 / 0.17 of it at k = 1 / 5 / 20.
"""
import numpy as np
import pytest

import score_ref64 as sr
import top_ref64 as tr

pytestmark = pytest.mark.gpu

V_BIG = 50257
GUARD = 4096
FILL = 0xFF
KS = [1, 5, 20]


def _big_rows():
    """the eight rows of the V = 50257 case, with what each is there for"""
    V = V_BIG
    rng = np.random.default_rng(20)
    x = np.zeros((8, V), np.float32)
    x[0] = rng.standard_normal(V)                                   # noise
    x[1] = 0.5                                                      # every value equal
    x[2] = rng.standard_normal(V)                                   # 29 ties at the top, head and tail included
    cols = np.concatenate([[0, 1, V - 2, V - 1], rng.choice(np.arange(2, V - 2), 25, replace=False)])
    x[2, cols] = x[2].max()
    x[3] = rng.standard_normal(V)                                   # ten distinct values, then a 40-way tie
    free = rng.choice(np.arange(V - 1), 49, replace=False)
    x[3, free[:10]] = 20.0 + np.arange(10, dtype=np.float32)
    x[3, np.concatenate([free[10:], [V - 1]])] = 12.5
    x[4] = -1.0 - np.abs(rng.standard_normal(V))                    # only signed zeros are not negative
    z = rng.choice(V, 60, replace=False)
    x[4, z[:30]] = np.float32(-0.0)
    x[4, z[30:]] = np.float32(0.0)
    x[5] = np.arange(V, dtype=np.float32) * 1e-3                     # ascending ramp: the top k are the tail
    x[6] = -np.arange(V, dtype=np.float32) * 1e-3                    # descending ramp
    x[7] = rng.standard_normal(V)                                   # one logit 80 above the noise
    x[7, 31337] = 80.0
    return x


def _small_rows(V):
    rng = np.random.default_rng(V)
    x = rng.standard_normal((3, V)).astype(np.float32)
    x[1] = -2.25                      # all equal
    x[2, [V - 1, 0, V // 2]] = 3.0    # ties over the head, the middle and the tail
    return x


@pytest.fixture(scope="module")
def big():
    x = _big_rows()
    return x, {k: tr.topk64(x, k) for k in KS}


class _Dev:
    def __init__(self, hip, x):
        self.hip, self.x = hip, x
        self.rows, self.V = x.shape
        self.dx = hip.DeviceBuffer.from_array(x)

    def launch(self, k, active=None, targets=None, want_lse=True, kbuf=None):
        """one launch into 0xFF-filled outputs; returns (rc, ids, lps, target_lp, lse) as raw bytes"""
        hip, n = self.hip, self.rows
        kbuf = k if kbuf is None else kbuf
        sizes = dict(ids=n * kbuf * 4, lps=n * kbuf * 4, tlp=n * 4, lse=n * 4)
        bufs = {name: hip.DeviceBuffer.from_array(np.full(sz + GUARD, FILL, np.uint8)) for name, sz in sizes.items()}
        act = hip.DeviceBuffer.from_array(np.asarray(active, np.int32)) if active is not None else None
        tgt = hip.DeviceBuffer.from_array(np.asarray(targets, np.int32)) if targets is not None else None
        rc = hip.lib().hpa_top_logprobs(self.dx.ptr, n, self.V, k, act.ptr if act else None, tgt.ptr if tgt else None,
                                        bufs["ids"].ptr, bufs["lps"].ptr, bufs["tlp"].ptr if tgt else None,
                                        bufs["lse"].ptr if want_lse else None)
        hip.check(hip.lib().hpa_synchronize())
        raw = {name: bufs[name].download(sizes[name] + GUARD, np.uint8) for name in sizes}
        for name, sz in sizes.items():
            assert (raw[name][sz:] == FILL).all(), f"{name}: written behind the last row"
        return rc, {name: raw[name][:sz] for name, sz in sizes.items()}


def _check(x, k, out, ref, targets=None, rows=None):
    n = x.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    ids = out["ids"].view(np.int32).reshape(n, k)
    lps = out["lps"].view(np.float32).reshape(n, k)
    rid, rlp = ref
    assert np.array_equal(ids[rows], rid[rows]), (ids[rows], rid[rows])
    err = np.abs(lps.astype(np.float64) - rlp)
    bd = tr.bound(x, rid)
    worst = float((err[rows] / bd[rows]).max())
    assert np.all(err[rows] <= bd[rows]), worst
    assert np.all(np.diff(lps[rows], axis=-1) <= 0)
    lse = out["lse"].view(np.float32)
    lse64 = sr.lse64(x)
    assert np.all(np.abs(lse.astype(np.float64) - lse64)[rows] <= (4e-6 + 2.0 ** -22 * np.abs(lse64))[rows])
    if targets is not None:
        tlp = out["tlp"].view(np.float32)
        terr = np.abs(tlp.astype(np.float64) - sr.logprob64(x, targets))
        assert np.all(terr[rows] <= sr.kernel_bound(x, targets)[rows])
        assert np.all(tlp[rows][np.asarray(targets)[rows] < 0] == 0.0)
    return worst


@pytest.mark.parametrize("k", KS)
def test_big_rows(hip, big, k):
    x, refs = big
    rid = refs[k][0]
    dev = _Dev(hip, x)
    # targets: a top column, a column outside the top k, none -- in turn over the rows
    not_top = np.array([int(np.setdiff1d(np.arange(64), rid[r])[0]) for r in range(8)])
    targets = np.where(np.arange(8) % 3 == 0, rid[:, k - 1], np.where(np.arange(8) % 3 == 1, not_top, -1)).astype(np.int32)
    rc, out = dev.launch(k, targets=targets)
    assert rc == 0
    worst = _check(x, k, out, refs[k], targets)
    print(f"V={V_BIG} k={k}: worst |lp err| / bound = {worst:.3f}")
    lps = out["lps"].view(np.float32).reshape(8, k)
    assert np.all(np.abs(lps[1] + np.log(float(V_BIG))) <= tr.bound(x, rid)[1])  # the all-equal row: -log V
    assert np.array_equal(out["ids"].view(np.int32).reshape(8, k)[1], np.arange(k))
    rc2, out2 = dev.launch(k, targets=targets)
    assert rc2 == 0
    for name in out:
        assert np.array_equal(out[name], out2[name]), f"{name}: a second launch differs"


def test_the_answer_does_not_depend_on_the_slice_count(hip, big):
    """the fewest slices a wave's registers allow (50), the most one wave merges
    (64), and counts the four-wave merge takes (100, 256): the same ids, every
    log-probability within the bound"""
    x, refs = big
    k, n = 20, 8
    dx = hip.DeviceBuffer.from_array(x)
    ws_bytes = n * 256 * (12 + 8 * k)
    ws = hip.DeviceBuffer(ws_bytes)
    for slices in (50, 64, 100, 256):
        ids, lps, lse = (hip.DeviceBuffer(n * k * 4), hip.DeviceBuffer(n * k * 4), hip.DeviceBuffer(n * 4))
        hip.check(hip.lib().hpa_top_logprobs_ws(dx.ptr, n, V_BIG, k, None, None, ids.ptr, lps.ptr, None, lse.ptr,
                                                ws.ptr, ws_bytes, slices), "hpa_top_logprobs_ws")
        hip.check(hip.lib().hpa_synchronize())
        out = dict(ids=ids.download((n, k), np.int32).view(np.uint8).reshape(-1),
                   lps=lps.download((n, k)).view(np.uint8).reshape(-1), lse=lse.download(n).view(np.uint8))
        _check(x, k, out, refs[k])
    # 49 slices of 50257 columns do not fit a wave's registers, 257 lists not the merge: refused
    assert hip.lib().hpa_top_logprobs_ws(dx.ptr, n, V_BIG, k, None, None, ids.ptr, lps.ptr, None, lse.ptr, ws.ptr,
                                         ws_bytes, 49) != 0
    assert hip.lib().hpa_top_logprobs_ws(dx.ptr, n, V_BIG, k, None, None, ids.ptr, lps.ptr, None, lse.ptr, ws.ptr,
                                         ws_bytes, 257) != 0


@pytest.mark.parametrize("k", KS)
def test_inactive_rows_keep_their_fill(hip, big, k):
    x, refs = big
    dev = _Dev(hip, x)
    active = np.array([1, 0, 2, -1, 1, 0, 1, 1], np.int32)
    targets = np.array([5, 6, -1, 8, 9, 10, 11, 31337], np.int32)
    rc, out = dev.launch(k, active=active, targets=targets)
    assert rc == 0
    on = np.flatnonzero(active > 0)
    _check(x, k, out, refs[k], targets, rows=on)
    for name, per in (("ids", k * 4), ("lps", k * 4), ("tlp", 4), ("lse", 4)):
        rows = out[name].reshape(8, per)
        assert (rows[active <= 0] == FILL).all(), name
        assert not (rows[on] == FILL).all(axis=1).any(), name


@pytest.mark.parametrize("V", [33, 20])
@pytest.mark.parametrize("k", KS)
def test_small_rows(hip, V, k):
    x = _small_rows(V)
    dev = _Dev(hip, x)
    ref = tr.topk64(x, k)
    targets = np.array([ref[0][0, 0], V - 1, -1], np.int32)
    rc, out = dev.launch(k, targets=targets)
    assert rc == 0
    _check(x, k, out, ref, targets)
    rc2, out2 = dev.launch(k, targets=targets)
    assert rc2 == 0 and all(np.array_equal(out[n], out2[n]) for n in out)
    # no optional output at all
    rc3, out3 = dev.launch(k, want_lse=False)
    assert rc3 == 0
    assert np.array_equal(out3["ids"], out["ids"]) and np.array_equal(out3["lps"], out["lps"])
    assert (out3["lse"] == FILL).all() and (out3["tlp"] == FILL).all()


def test_refusals_write_nothing(hip):
    x = _small_rows(20)
    dev = _Dev(hip, x)
    L = hip.lib()
    for k in (0, 21, -3):
        rc, out = dev.launch(k, kbuf=21, targets=np.zeros(3, np.int32))
        assert rc != 0, k
        assert all((out[n] == FILL).all() for n in out), k
    small = _Dev(hip, _small_rows(20)[:, :12].copy())  # k > V
    rc, out = small.launch(20, targets=np.zeros(3, np.int32))
    assert rc != 0 and all((out[n] == FILL).all() for n in out)
    ids, lps = hip.DeviceBuffer(3 * 5 * 4), hip.DeviceBuffer(3 * 5 * 4)
    assert L.hpa_top_logprobs(None, 3, 20, 5, None, None, ids.ptr, lps.ptr, None, None) != 0
    assert L.hpa_top_logprobs(dev.dx.ptr, 3, 20, 5, None, None, None, lps.ptr, None, None) != 0
    assert L.hpa_top_logprobs(dev.dx.ptr, 3, 20, 5, None, None, ids.ptr, None, None, None) != 0
    assert L.hpa_top_logprobs(dev.dx.ptr, 0, 20, 5, None, None, ids.ptr, lps.ptr, None, None) != 0
    # target_lp without targets
    assert L.hpa_top_logprobs(dev.dx.ptr, 3, 20, 5, None, None, ids.ptr, lps.ptr, lps.ptr, None) != 0
    rc, out = dev.launch(5)  # and the library still works
    assert rc == 0
    _check(x, 5, out, tr.topk64(x, 5))
