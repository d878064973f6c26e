"""hpa_sample_filtered (temperature / top-k / top-p per row) against the
float64 restatement of its rules (sample_ref64.py).

Tolerance, per row and from the reference alone: tol = max(4 e, 2^-20), e the
largest difference between the row's float64 cdf and the cdf of its fp32 exp
terms summed sequentially in fp32 (sample_ref64.tolerance).  The largest tol
of a case is printed.

Every active row of every launch is checked:
  1. n_kept / cut: M[n-1] >= P - tol, M[n-2] < P + tol, n <= top-k size,
     n == top-k size where P = 1, cut bit-equal to the logit at canonical
     position n - 1; on randn40 / equal / spike the interval admits one n and
     the device must report it;
  2. the id lies in the kept set of the device's own (n_kept, cut) and
     c[prev kept] - tol <= u < c[pick] + tol on the float64 index-order cdf;
  3. states equal the Python xorshift's bit for bit, tokens == next, pos += 1.
"""
import numpy as np
import pytest

import sample_ref64 as sr

pytestmark = pytest.mark.gpu

B, DRAWS = 12, 4
EXACT_KINDS = ("randn40", "equal", "spike")


def _logits(kind, B, V, rng):
    if kind.startswith("randn"):
        return (rng.standard_normal((B, V)) * float(kind[5:])).astype(np.float32)
    if kind == "quant":  # repeated values: tie groups everywhere
        return (np.round(rng.standard_normal((B, V)) * 4) / 4).astype(np.float32)
    if kind == "equal":
        return np.zeros((B, V), np.float32)
    if kind == "spike":  # one dominant logit
        x = (rng.standard_normal((B, V)) - 30).astype(np.float32)
        x[np.arange(B), rng.integers(0, V, B)] = 5.0
        return x
    if kind == "ramp":
        return np.tile(np.linspace(-20, 0, V, dtype=np.float32), (B, 1))
    raise ValueError(kind)


def _settings(table, V):
    """12 rows, each with its own (T, k, P); between them the two tables cover
    k in {1, 2, 50, V-1, V, V+7}, P in {1, .999, .9, .5, 1e-6}, T in {0, .5, 1, 1.7}"""
    a = [(1.0, 0, 1.0), (0.0, 0, 1.0), (0.5, 1, 1.0), (1.7, 2, 0.9), (1.0, 50, 1.0), (0.5, 50, 0.9),
         (1.7, V - 1, 0.999), (1.0, V, 0.5), (0.5, V + 7, 0.999), (1.7, 0, 0.5), (1.0, 0, 1e-6), (0.5, 0, 0.9)]
    b = [(1.7, 50, 1.0), (1.0, 0, 0.999), (0.0, 50, 0.5), (0.5, 2, 1.0), (1.0, 1, 0.5), (1.7, V - 1, 1.0),
         (0.5, 0, 0.5), (1.0, 50, 0.9), (1.7, 0, 0.9), (0.5, V - 1, 1e-6), (1.0, 2, 0.999), (1.7, V + 7, 0.5)]
    rows = a if table == "a" else b
    return (np.array([r[0] for r in rows], np.float32), np.array([max(r[1], 0) for r in rows], np.int32),
            np.array([r[2] for r in rows], np.float32))


class _Dev:
    """device buffers of one launch shape"""

    def __init__(self, hip, x, T, k, P, seeds):
        n = x.shape[0]
        self.hip, self.n, self.V = hip, n, x.shape[1]
        self.x = hip.DeviceBuffer.from_array(x)
        self.T = hip.DeviceBuffer.from_array(np.asarray(T, np.float32))
        self.k = hip.DeviceBuffer.from_array(np.asarray(k, np.int32))
        self.P = hip.DeviceBuffer.from_array(np.asarray(P, np.float32))
        self.st = hip.DeviceBuffer.from_array(np.asarray(seeds, np.uint64))
        self.next = hip.DeviceBuffer.from_array(np.full(n, -5, np.int32))
        self.tok = hip.DeviceBuffer.from_array(np.full(n, -7, np.int32))
        self.pos = hip.DeviceBuffer.from_array(np.arange(n, dtype=np.int32) * 3)
        self.nk = hip.DeviceBuffer.from_array(np.full(n, -9, np.int32))
        self.cut = hip.DeviceBuffer.from_array(np.full(n, -123.0, np.float32))

    def launch(self, active=None, outputs=True):
        act = self.hip.DeviceBuffer.from_array(np.asarray(active, np.int32)) if active is not None else None
        self.hip.check(self.hip.lib().hpa_sample_filtered(
            self.x.ptr, self.n, self.V, self.T.ptr, self.k.ptr, self.P.ptr, self.st.ptr, self.next.ptr,
            self.tok.ptr, self.pos.ptr, act.ptr if act else None, self.nk.ptr if outputs else None,
            self.cut.ptr if outputs else None), "hpa_sample_filtered")
        return self.get()

    def get(self):
        n = self.n
        return dict(next=self.next.download(n, np.int32), tok=self.tok.download(n, np.int32),
                    pos=self.pos.download(n, np.int32), nk=self.nk.download(n, np.int32),
                    cut=self.cut.download(n, np.float32), st=self.st.download(n, np.uint64))


def _run_case(hip, kind, V, table, seed):
    x = _logits(kind, B, V, np.random.default_rng(seed))
    T, k, P = _settings(table, V)
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(1337 + seed)
    dev = _Dev(hip, x, T, k, P, seeds)
    states = [int(s) for s in seeds]
    tols = [sr.tolerance(x[b], T[b]) if T[b] > 0 else 0.0 for b in range(B)]
    print(f"[sample_filtered] {kind} V={V} table {table}: largest tol {max(tols):.3e}")
    for d in range(DRAWS):
        out = dev.launch()
        assert np.array_equal(out["next"], out["tok"])
        assert np.array_equal(out["pos"], np.arange(B) * 3 + d + 1)
        for b in range(B):
            states[b], u = sr.coin(states[b])
            assert int(out["st"][b]) == states[b], (b, d)
            nxt, n, cut = int(out["next"][b]), int(out["nk"][b]), out["cut"][b]
            assert 0 <= nxt < V
            if T[b] == 0 or k[b] == 1:  # greedy rows and k = 1 rows: exactly the argmax, lowest index
                assert nxt == int(np.argmax(x[b])), (b, nxt)
                assert n == 1 and cut == x[b].max(), (b, n, cut)
                if T[b] == 0:
                    continue
            sr.check_cut(x[b], T[b], k[b], P[b], n, cut, tols[b], exact=kind in EXACT_KINDS)
            sr.check_pick(x[b], T[b], n, cut, u, nxt, tols[b])


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_small_vocabularies_on_wave_histogram_and_chunk_edges(hip, V):
    _run_case(hip, "randn3", V, "a", V)
    _run_case(hip, "quant", V, "b", V + 1)


@pytest.mark.parametrize("kind,table", [("randn1", "a"), ("randn3", "b"), ("randn40", "a"), ("quant", "b"),
                                        ("equal", "a"), ("spike", "b"), ("ramp", "a")])
def test_gpt2_vocabulary_every_kind(hip, kind, table):
    """V = 50257 is odd: rows are 4-byte aligned only (head and tail peeled)"""
    _run_case(hip, kind, 50257, table, len(kind) + ord(kind[0]))


@pytest.mark.parametrize("kind,V", [("quant", 50257), ("quant", 4097), ("equal", 50257), ("equal", 257)])
def test_top_k_through_a_tie_group_keeps_the_lowest_indices(hip, kind, V):
    x = _logits(kind, B, V, np.random.default_rng(5))
    ks = []
    for b in range(B):  # the first k >= 3 + b whose cut falls inside a tie group
        order = sr.Row(x[b], 1.0, 0).order
        k = 3 + b
        while not (x[b][order[k - 1]] == x[b][order[k]]):
            k += 1
        ks.append(k)
    T = np.full(B, 0.5, np.float32)
    P = np.ones(B, np.float32)
    dev = _Dev(hip, x, T, ks, P, np.arange(B, dtype=np.uint64) + np.uint64(77))
    states = [77 + b for b in range(B)]
    for _ in range(DRAWS):
        out = dev.launch()
        for b in range(B):
            states[b], u = sr.coin(states[b])
            n, cut = int(out["nk"][b]), out["cut"][b]
            row = sr.check_cut(x[b], T[b], ks[b], 1.0, n, cut, 2.0 ** -20)
            assert n == ks[b]
            kept = sr.kept_indices(x[b], n, cut)
            assert np.array_equal(kept, np.sort(row.order[:ks[b]]))  # the lowest indices of the tie group
            sr.check_pick(x[b], T[b], n, cut, u, int(out["next"][b]), sr.tolerance(x[b], T[b]))


def test_top_p_through_equal_logits(hip):
    V = 50257
    x = _logits("equal", B, V, None)
    T = np.array([0.5, 1.0, 1.7] * 4, np.float32)
    P = np.full(B, 0.5, np.float32)
    dev = _Dev(hip, x, T, np.zeros(B, np.int32), P, np.arange(B, dtype=np.uint64) + np.uint64(3))
    out = dev.launch()
    for b in range(B):
        tol = sr.tolerance(x[b], T[b])
        sr.check_cut(x[b], T[b], 0, 0.5, int(out["nk"][b]), out["cut"][b], tol, exact=True)
        assert out["cut"][b] == 0.0 and out["nk"][b] == (V + 1) // 2
        assert out["next"][b] < out["nk"][b]  # the lowest indices are the kept ones


def test_inactive_rows_untouched_and_greedy_rows_draw_a_coin(hip):
    V = 4097
    x = _logits("randn3", B, V, np.random.default_rng(8))
    T, k, P = _settings("a", V)
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(99)
    dev = _Dev(hip, x, T, k, P, seeds)
    active = np.array([1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0], np.int32)
    out = dev.launch(active=active)
    for b in range(B):
        if active[b]:
            s, u = sr.coin(int(seeds[b]))
            assert int(out["st"][b]) == s  # once per call, the greedy row (T[1] = 0) included
            assert out["pos"][b] == 3 * b + 1 and out["tok"][b] == out["next"][b]
            if T[b] > 0:
                sr.check_pick(x[b], T[b], int(out["nk"][b]), out["cut"][b], u, int(out["next"][b]),
                              sr.tolerance(x[b], T[b]))
        else:
            assert out["next"][b] == -5 and out["tok"][b] == -7 and out["pos"][b] == 3 * b
            assert out["st"][b] == seeds[b] and out["nk"][b] == -9 and out["cut"][b] == np.float32(-123.0)
    assert T[1] == 0 and active[1] == 1 and out["next"][1] == int(np.argmax(x[1]))


@pytest.mark.parametrize("kind,V", [("randn3", 50257), ("quant", 4097)])
def test_null_outputs_and_repeated_launches_give_the_same_ids(hip, kind, V):
    x = _logits(kind, B, V, np.random.default_rng(21))
    T, k, P = _settings("b", V)
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(5)
    first = _Dev(hip, x, T, k, P, seeds).launch()
    again = _Dev(hip, x, T, k, P, seeds).launch()  # the same inputs and states: identical results
    for key in ("next", "nk", "st"):
        assert np.array_equal(first[key], again[key]), key
    assert first["cut"].tobytes() == again["cut"].tobytes()
    bare = _Dev(hip, x, T, k, P, seeds).launch(outputs=False)  # n_kept / cut NULL: the same ids
    assert np.array_equal(bare["next"], first["next"]) and np.array_equal(bare["st"], first["st"])
    assert (bare["nk"] == -9).all()


def test_out_of_range_settings_are_read_as_defaults(hip):
    """the raw entry sanitises: T < 0 / non-finite -> 1, k < 0 -> 0, P outside (0, 1] -> 1"""
    V = 257
    x = _logits("randn3", B, V, np.random.default_rng(2))
    T = np.array([-1, np.nan, np.inf, 1, 1, 1, 1, 1, -np.inf, 1, 1, 1], np.float32)
    k = np.array([0, 0, 0, -4, 0, 0, 0, -2 ** 31, 0, 0, 0, 0], np.int32)
    P = np.array([1, 1, 1, 1, 0, 1.5, np.nan, -1, np.inf, 1, 1, 1], np.float32)
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(41)
    out = _Dev(hip, x, T, k, P, seeds).launch()
    for b in range(B):
        _, u = sr.coin(int(seeds[b]))
        assert out["nk"][b] == V and out["cut"][b] == x[b].min()
        sr.check_pick(x[b], 1.0, V, out["cut"][b], u, int(out["next"][b]), sr.tolerance(x[b], 1.0))
