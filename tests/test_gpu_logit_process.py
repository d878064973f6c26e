"""hpa_logits_process called directly, against logit_ref64 (the float64
restatement of its rules), then hpa_argmax_final over its partials.

Tolerance, per element and from the reference alone: tol = 2^-21 S with S =
|x'| + |f c| + |p| + |bias| (logit_ref64); a reference -inf must be -inf.  The
picked id must be the reference winner exactly: test_logit_ref64.py shows that
every row's winner leads by more than 2 tol or ties exactly.  The largest
error / tol ratio of a case is printed.

Every output buffer is filled with 0xFF and followed by a guard region; an
inactive row keeps the fill, its next id and its position.

The samplers are then run on a processed row that holds -inf entries (bans):
hpa_sample_filtered against sample_ref64.check_pick_any, hpa_sample_final
against the reference sampler, 200 coins each; a banned id is never drawn.
"""
import numpy as np
import pytest

import logit_ref64 as lr
import oracle_ctypes as oc
import sample_ref64 as sr

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xFF


class _Dev:
    """the device buffers of one kernel_case; outputs 0xFF-filled with a guard behind"""

    def __init__(self, hip, case):
        self.hip, self.case = hip, case
        self.n, self.V = case["x"].shape
        self.Mp = (self.n + 15) // 16 * 16
        buf = hip.DeviceBuffer.from_array
        self.x = buf(case["x"])
        self.counts = buf(case["counts"])
        self.r, self.p, self.f = buf(case["r"]), buf(case["p"]), buf(case["f"])
        self.ids, self.vals, self.nb = buf(case["bias_ids"]), buf(case["bias_vals"]), buf(case["bias_n"])
        self.active = buf(case["active"])
        self.max_slices = max(64, hip.lib().hpa_logits_process_slices(self.n, self.V, 256))
        self.out_bytes = self.n * self.V * 4
        self.part_bytes = self.max_slices * self.Mp * 8
        self.out = hip.DeviceBuffer(self.out_bytes + GUARD)
        self.part = hip.DeviceBuffer(self.part_bytes + GUARD)
        self.next = hip.DeviceBuffer(self.n * 4 + GUARD)
        self.pos = hip.DeviceBuffer(self.n * 4)
        self.launches = 0

    def launch(self, slices=0, store=True):
        hip, n = self.hip, self.n
        for b in (self.out, self.part, self.next):
            b.upload(np.full(b.nbytes, FILL, np.uint8))
        self.pos.upload(np.arange(n, dtype=np.int32) * 5)
        hip.check(hip.lib().hpa_logits_process(self.x.ptr, n, self.V, self.counts.ptr, self.r.ptr, self.p.ptr,
                                               self.f.ptr, self.ids.ptr, self.vals.ptr, self.nb.ptr, self.active.ptr,
                                               self.out.ptr if store else None, self.part.ptr, self.Mp, slices),
                  "hpa_logits_process")
        s = slices if slices > 0 else hip.lib().hpa_logits_process_slices(n, self.V, _cus(hip))
        assert 1 <= s <= self.max_slices
        hip.check(hip.lib().hpa_argmax_final(self.part.ptr, s, self.Mp, n, self.next.ptr, None, self.pos.ptr,
                                             self.active.ptr), "hpa_argmax_final")
        out = self.out.download(self.out_bytes + GUARD, np.uint8)
        part = self.part.download(self.part_bytes + GUARD, np.uint8)
        nxt = self.next.download(self.n * 4 + GUARD, np.uint8)
        assert (out[self.out_bytes:] == FILL).all() and (nxt[n * 4:] == FILL).all()  # guards
        assert (part[s * self.Mp * 8:] == FILL).all()  # nothing past the slices in use, guard included
        return dict(out=out[:self.out_bytes].view(np.float32).reshape(n, self.V), raw_out=out[:self.out_bytes],
                    part=part[:s * self.Mp * 8].view(np.uint32).reshape(s, self.Mp, 2),
                    next=nxt[:n * 4].view(np.int32), pos=self.pos.download(n, np.int32), slices=s)


def _cus(hip):
    import ctypes
    n = ctypes.c_int()
    hip.check(hip.lib().hpa_device_info(None, 0, ctypes.byref(n), None), "device_info")
    return n.value


@pytest.mark.parametrize("V,kinds", lr.KERNEL_CASES)
def test_logits_process_matches_float64(hip, V, kinds):
    case = lr.kernel_case(V, kinds)
    ref = lr.kernel_reference(case)
    dev = _Dev(hip, case)
    got = dev.launch()
    n = len(kinds)
    worst = 0.0
    for b in range(n):
        y, tol = ref[b]
        row_bytes = got["raw_out"][b * V * 4:(b + 1) * V * 4]
        if kinds[b] == lr.INACTIVE:  # processed row, partials, next id and position keep their fill
            assert (row_bytes == FILL).all()
            assert (got["part"][:, b, :] == 0xFFFFFFFF).all()
            assert got["next"][b] == -1 and got["pos"][b] == 5 * b
            continue
        worst = max(worst, lr.assert_close(got["out"][b], y, tol, (V, b, kinds[b])))
        if kinds[b] == lr.NEUTRAL:  # every step is exact: the raw bits
            assert row_bytes.tobytes() == case["x"][b].tobytes()
        assert got["next"][b] == lr.winner(y), (V, b, kinds[b], got["next"][b], lr.winner(y))
        assert got["pos"][b] == 5 * b + 1
    print(f"[logits_process] V={V} kinds={kinds} slices={got['slices']}: largest error / tol {worst:.3f}")

    again = dev.launch()  # a second launch: bit-identical
    assert again["raw_out"].tobytes() == got["raw_out"].tobytes()
    assert again["part"].tobytes() == got["part"].tobytes()
    assert np.array_equal(again["next"], got["next"])

    nostore = dev.launch(store=False)  # no processed rows asked for: the same ids, nothing stored
    assert np.array_equal(nostore["next"], got["next"]) and (nostore["raw_out"] == FILL).all()
    assert nostore["part"].tobytes() == got["part"].tobytes()

    for s in (1, 7, 33):  # one slice, odd slice counts: edges fall anywhere
        forced = dev.launch(slices=s)
        assert forced["slices"] == s
        assert np.array_equal(forced["next"], got["next"]), (s, forced["next"], got["next"])
        assert forced["raw_out"].tobytes() == got["raw_out"].tobytes()


def test_slices_is_pure_and_bounded(hip):
    L = hip.lib()
    assert L.hpa_logits_process_slices(0, 50257, 256) == 0 and L.hpa_logits_process_slices(8, 0, 256) == 0
    for B in (1, 8, 64, 256):
        for V in (1, 1000, 1003, 50257, 200000):
            s = L.hpa_logits_process_slices(B, V, 256)
            assert s >= 1 and s == L.hpa_logits_process_slices(B, V, 256)
            assert (V // 4 + s - 1) // s * 4 + 8 <= 65536  # a slice fits the kernel's bitmap
            assert s == 1 or V // s >= 1000  # no slice far under one load per lane
    assert L.hpa_logits_process_slices(8, 50257, 256) * 8 >= 256  # B = 8 still fills the CUs
    assert L.hpa_logits_process_slices(64, 50257, 256) <= 16  # B = 64 is not over-split


def test_too_few_slices_for_the_row_are_refused(hip):
    V = 200000  # in one slice: over the kernel's bitmap.  Buffers of the full size all the same
    buf = hip.DeviceBuffer.from_array
    x, counts, one = buf(np.zeros((1, V), np.float32)), buf(np.zeros((1, V), np.uint16)), buf(np.ones(1, np.float32))
    part = buf(np.zeros(16 * 2 * 4, np.float32))
    with pytest.raises(RuntimeError):
        hip.check(hip.lib().hpa_logits_process(x.ptr, 1, V, counts.ptr, one.ptr, one.ptr, one.ptr, None, None, None,
                                               None, None, part.ptr, 16, 1), "process")
    hip.check(hip.lib().hpa_logits_process(x.ptr, 1, V, counts.ptr, one.ptr, one.ptr, one.ptr, None, None, None,
                                           None, None, part.ptr, 16, 4), "process")  # four slices fit
    hip.check(hip.lib().hpa_synchronize(), "synchronize")


# ---------------------------------------------------------------- samplers on rows with bans
def _processed_rows(hip, B, V, seed):
    """B processed rows out of the kernel: penalties and a bias list whose
    first 120 entries are bans (the raw top 40 among them)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, V)) * 2).astype(np.float32)
    case = dict(x=x, counts=np.zeros((B, V), np.uint16), r=np.full(B, 1.2, np.float32),
                p=np.full(B, 0.3, np.float32), f=np.full(B, 0.05, np.float32),
                bias_ids=np.zeros((B, lr.BIAS_MAX), np.int32), bias_vals=np.zeros((B, lr.BIAS_MAX), np.float32),
                bias_n=np.full(B, lr.BIAS_MAX, np.int32), active=np.ones(B, np.int32))
    banned = []
    for b in range(B):
        case["counts"][b, rng.permutation(V)[:150]] = rng.integers(1, 6, 150)
        top = np.argsort(-x[b])[:40]
        rest = np.setdiff1d(rng.permutation(V), top, assume_unique=True)[:lr.BIAS_MAX - 40]
        case["bias_ids"][b] = np.concatenate([top, rest])
        case["bias_vals"][b] = rng.uniform(-2, 2, lr.BIAS_MAX).astype(np.float32)
        case["bias_vals"][b, :120] = -np.inf
        banned.append(set(int(i) for i in case["bias_ids"][b, :120]))
    dev = _Dev(hip, case)
    got = dev.launch()
    for b, (y, tol) in enumerate(lr.kernel_reference(case)):
        lr.assert_close(got["out"][b], y, tol)
        assert np.isneginf(got["out"][b]).sum() == 120
    return dev, got["out"].copy(), banned


@pytest.mark.parametrize("V", [1000, 1003])
def test_sample_filtered_on_rows_with_bans(hip, V):
    B, draws = 8, 25  # 200 coins
    dev, rows, banned = _processed_rows(hip, B, V, seed=V)
    T = np.array([1.0, 0.7, 1.5, 1.0, 0.0, 1.0, 0.5, 2.0], np.float32)
    k = np.array([0, 0, 50, 0, 0, V - 1, 5, 0], np.int32)  # V - 1 > the columns left: the cut falls among the bans
    P = np.array([1.0, 0.9, 1.0, 0.5, 1.0, 1.0, 0.95, 0.999], np.float32)
    buf = hip.DeviceBuffer.from_array
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(4242 + V)
    d_T, d_k, d_P, d_st = buf(T), buf(k), buf(P), buf(seeds)
    d_next, d_pos = buf(np.full(B, -5, np.int32)), buf(np.zeros(B, np.int32))
    states = [int(s) for s in seeds]
    tols = [sr.tolerance(rows[b], T[b]) if T[b] > 0 else 0.0 for b in range(B)]
    print(f"[sample_filtered on bans] V={V}: largest tol {max(tols):.3e}")
    for d in range(draws):
        hip.check(hip.lib().hpa_sample_filtered(dev.out.ptr, B, V, d_T.ptr, d_k.ptr, d_P.ptr, d_st.ptr, d_next.ptr,
                                                None, d_pos.ptr, None, None, None), "hpa_sample_filtered")
        ids = d_next.download(B, np.int32)
        for b in range(B):
            states[b], u = sr.coin(states[b])
            assert 0 <= ids[b] < V and int(ids[b]) not in banned[b], (d, b, ids[b])
            assert np.isfinite(rows[b, ids[b]])
            sr.check_pick_any(rows[b], T[b], int(k[b]), P[b], u, int(ids[b]), tols[b])
    assert np.array_equal(d_pos.download(B, np.int32), np.full(B, draws))
    assert np.array_equal(d_st.download(B, np.uint64), np.array(states, np.uint64))


@pytest.mark.parametrize("V", [1000, 1003])
def test_sample_final_on_rows_with_bans(hip, V):
    B, draws = 8, 25  # 200 coins
    dev, rows, banned = _processed_rows(hip, B, V, seed=7 + V)
    buf = hip.DeviceBuffer.from_array
    d_st = buf(np.arange(B, dtype=np.uint64) + np.uint64(99))
    d_next = buf(np.full(B, -5, np.int32))
    sampler = oc.Sampler(B, seed=99)
    for d in range(draws):
        hip.check(hip.lib().hpa_sample_final(dev.out.ptr, B, V, d_st.ptr, d_next.ptr, None, None, None),
                  "hpa_sample_final")
        ids = d_next.download(B, np.int32)
        want = sampler.sample(rows)
        assert np.array_equal(ids, want), (d, ids, want)
        for b in range(B):
            assert int(ids[b]) not in banned[b], (d, b, ids[b])
