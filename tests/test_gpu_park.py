"""Parking (gpt2_decode_park / gpt2_decode_unpark): a sequence's K/V pages and
everything else that belongs to it go to host memory and come back, into the
same slot or another one, bit for bit.

The SMALL config of tests/test_gpu_serving.py, B = 4, every kv dtype (the fp8
pool with non-unit scales), P at the dtype's smallest engine page size and at
64.  The engines run over a caller's BlockManager so the tests can read the
sequences' page lists.  Whatever a park / unpark pair moves is compared as
bits against a control run on a fresh engine that never parked; where a
sequence continues in another slot its logits are held to LOGIT_TOL = 2e-4 of
the oracle PagedDecoder fed the full history (fp32 pools, as
tests/test_gpu_fork.py).
"""

import numpy as np
import pytest

import oracle_ctypes as oc
import pool_marks as pm
import synth

pytestmark = pytest.mark.gpu
SMALL = dict(maxT=256, V=1000, L=2, NH=2, C=128)
LOGIT_TOL = 2e-4
B = 4
KV = {"f32": 0, "bf16": 1, "fp8": 2}
POOLS = [(kv, P) for kv in KV for P in ({"f32": 8, "bf16": 8, "fp8": 16}[kv], 64)]
_params = {}


def _id(p):
    return f"{p[0]}-P{p[1]}"


def params_of(cfgd, seed=31):
    key = (tuple(sorted(cfgd.items())), seed)
    if key not in _params:
        _params[key] = synth.params(cfgd, seed=seed)
    return _params[key]


def fp8_scales(cfgd, seed=0):
    rng = np.random.default_rng([41, seed])
    shape = (cfgd["L"], cfgd["NH"])
    return (rng.uniform(0.01, 0.04, shape).astype(np.float32), rng.uniform(0.01, 0.04, shape).astype(np.float32))


class Eng:
    """an engine over a caller's block manager"""

    def __init__(self, hip, kv="f32", P=16, pages=None, cfgd=SMALL, scale_seed=0, batch=B):
        self.hip, self.cfgd, self.P, self.kv = hip, cfgd, P, kv
        per = cfgd["maxT"] // P
        self.bm = hip.BlockManager(cfgd["C"], max_prompts=batch, max_blocks=pages or batch * per, block_size=P,
                                   max_blocks_per_prompt=per)
        self.m = hip.Model(cfgd, params=params_of(cfgd))
        self.m.set_manager(self.bm)
        self.m.decode_init(batch, P, cfgd["maxT"], kv_dtype=KV[kv])
        if kv == "fp8":
            self.m.set_kv_scales(*fp8_scales(cfgd, scale_seed))

    def next_ids(self):
        out = np.zeros(self.m.B, np.int32)
        self.hip.check(self.hip.lib().hpa_synchronize())
        self.hip.check(self.hip.lib().hpa_memcpy(out.ctypes.data, self.m.next_ptr(), out.nbytes), "next ids")
        return out

    def kv_rows(self, b):
        n = int(self.m.positions()[b])
        return [self.m.read_kv(l, b, n) for l in range(self.cfgd["L"])]

    def pages(self, b):
        return self.bm.pages(b)

    def state(self):
        """what a refusal must leave alone"""
        return (self.m.free_pages(), self.m.positions().tolist(), [self.pages(b) for b in range(self.m.B)],
                self.next_ids().tolist())

    def pool_shape(self):
        """an HpaKVPool of the engine's shape (hpa_park_bytes reads nothing else)"""
        s = self.hip.HpaKVPool()
        c = self.cfgd
        s.num_layers, s.num_heads, s.head_size, s.page_size, s.dtype = c["L"], c["NH"], c["C"] // c["NH"], self.P, KV[self.kv]
        s.elem_bytes = pm.ELEM_BYTES[KV[self.kv]]
        s.page_elems = pm.page_elems(c["NH"], self.P, s.head_size)
        return s

    def close(self):
        self.m.close()
        self.bm.close()


def same_kv(a, b):
    return len(a) == len(b) and all(np.array_equal(ka.view(np.uint32), kb.view(np.uint32)) and
                                    np.array_equal(va.view(np.uint32), vb.view(np.uint32))
                                    for (ka, va), (kb, vb) in zip(a, b))


def tokens(seed, n):
    return [int(t) for t in np.random.default_rng([53, seed]).integers(0, SMALL["V"], n)]


def set_mode(m, mode):
    """0 greedy, 1 multinomial, 2 filtered with per-sequence settings"""
    if mode:
        m.set_sampling(True, seed=4711, filtered=mode == 2)
    if mode == 2:
        for b in range(m.B):
            m.set_sampling_params(b, temperature=0.7 + 0.15 * b, top_k=30 + 7 * b, top_p=0.85 + 0.03 * b)


def snap(e, out, b=0):
    lg = e.m.logits()
    out.append(dict(logits=lg[b].copy(), next=int(e.next_ids()[b]), kv=e.kv_rows(b), pos=e.m.positions().copy()))


def assert_same_snaps(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["logits"].view(np.uint32), y["logits"].view(np.uint32)), (what, i, "logits")
        assert x["next"] == y["next"], (what, i, "next id", x["next"], y["next"])
        assert same_kv(x["kv"], y["kv"]), (what, i, "kv")
        assert np.array_equal(x["pos"], y["pos"]), (what, i, x["pos"], y["pos"])


# ---------------------------------------------------------------- 1. the same slot, bit for bit
def same_slot_script(hip, kv, P, n, mode, graph, park, setup=None, extra=None):
    """prefill slot 0 with n tokens, 3 steps, two ragged calls that leave slot 0
    out (a prompt into slot 1, released each time), 4 more device-fed steps.
    park: slot 0 is parked before the two calls and unparked while the second
    prompt still holds the lowest pages.  Returns (snapshots of slot 0, its page
    lists before the park and at the end)."""
    e = Eng(hip, kv, P)
    m = e.m
    if setup:
        setup(m)
    m.set_graph(graph)
    set_mode(m, mode)
    out = []
    more = (lambda: out[-1].update(extra(e))) if extra else (lambda: None)
    m.prefill_ragged([tokens(n, n), [], [], []])
    snap(e, out), more()
    for _ in range(3):
        m.step(None)
        snap(e, out), more()
    before = e.pages(0)
    assert len(before) == -(-(n + 3) // P)
    h = m.park(0) if park else None
    if park:
        assert m.positions()[0] == 0 and e.pages(0) == []
    m.prefill_ragged([[], tokens(1000 + n, P + 3), [], []])
    m.release(1)
    m.prefill_ragged([[], tokens(2000 + n, P + 1), [], []])  # two pages: the lowest free ones
    if park:
        m.unpark(h, 0)
        h.free()
    m.release(1)
    snap(e, out), more()
    for _ in range(4):
        m.step(None)
        snap(e, out), more()
    after = e.pages(0)
    e.close()
    return out, before, after


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["greedy", "multinomial", "filtered"])
@pytest.mark.parametrize("pool", POOLS, ids=_id)
def test_same_slot_bit_for_bit(hip, pool, mode, graph):
    kv, P = pool
    for n in (1, P, P + 1, 3 * P - 1):
        want, pages0, pages1 = same_slot_script(hip, kv, P, n, mode, graph, park=False)
        got, before, after = same_slot_script(hip, kv, P, n, mode, graph, park=True)
        assert pages0 == before and pages1[:len(pages0)] == pages0  # the control never moved
        assert len(after) == len(pages1)
        assert set(after[:len(before)]) != set(before), (n, before, after)  # it came back into other pages
        assert_same_snaps(want, got, (kv, P, n, mode, graph))
        assert want[-1]["pos"][0] == n + 7


# ---------------------------------------------------------------- 2. another slot
@pytest.mark.parametrize("pool", POOLS, ids=_id)
def test_unpark_into_another_slot(hip, pool):
    kv, P = pool
    e = Eng(hip, kv, P)
    m = e.m
    m.set_sampling(True, seed=99, filtered=True)
    m.set_sampling_params(0, temperature=0.8, top_k=40, top_p=0.9)
    m.set_penalties(0, repetition=1.3, presence=0.2, frequency=0.1, from_pos=2)  # processors off: settings only
    m.set_logit_bias(0, [3, 7, 900], [1.5, -np.inf, -0.25])
    prompt = tokens(7, P + 5)
    hist = list(prompt)
    oracle = None
    if kv == "f32":
        oracle = oc.PagedDecoder(params_of(SMALL), oc.cfg(SMALL["maxT"], SMALL["V"], SMALL["L"], SMALL["NH"], SMALL["C"]),
                                 1, P, SMALL["maxT"], page_seed=5)
        for t in prompt:
            _, o_logits = oracle.step(np.array([t], np.int32))
    fed = int(m.prefill_ragged([prompt, [], [], []])[0])
    for _ in range(2):
        if oracle:
            _, o_logits = oracle.step(np.array([fed], np.int32))
        hist.append(fed)
        fed = int(m.step(None)[0])
    n = len(hist)
    kv0, row0, state0 = e.kv_rows(0), m.logits()[0].copy(), m.sampler_state(0)
    if oracle:
        assert float(np.abs(row0 - o_logits[0]).max()) <= LOGIT_TOL
    settings = (m.sampling_params(0), m.penalties(0), [a.tolist() for a in m.logit_bias(0)])
    other = (m.sampling_params(2), m.penalties(2), [a.tolist() for a in m.logit_bias(2)])
    assert settings != other
    h = m.park(0)
    assert h.tokens == n and m.positions().tolist() == [0, 2, 2, 2]
    m.release(2)
    m.unpark(h, 2)
    assert m.positions().tolist() == [0, 2, n, 2]
    assert same_kv(e.kv_rows(2), kv0)
    assert np.array_equal(m.logits()[2].view(np.uint32), row0.view(np.uint32))
    assert int(e.next_ids()[2]) == fed and m.sampler_state(2) == state0
    assert (m.sampling_params(2), m.penalties(2), [a.tolist() for a in m.logit_bias(2)]) == settings
    assert np.isneginf(m.logit_bias(2)[1][1])
    worst = 0.0
    for _ in range(4):
        nxt = m.step(None)
        if oracle:
            _, o_logits = oracle.step(np.array([fed], np.int32))
            worst = max(worst, float(np.abs(m.logits()[2] - o_logits[0]).max()))
        fed = int(nxt[2])
    assert m.positions()[2] == n + 4
    assert same_kv([(k[:n], v[:n]) for k, v in e.kv_rows(2)], kv0)
    if oracle:
        print(f"PARK other slot {kv} P={P}: worst |logit - oracle| {worst:.2e}")
        assert worst <= LOGIT_TOL, worst
        oracle.close()
    h.free()
    e.close()


# ---------------------------------------------------------------- 3. handle reuse and keep
@pytest.mark.parametrize("pool", POOLS, ids=_id)
def test_handle_reuse_and_keep(hip, pool):
    kv, P = pool

    def run(checkpoint):
        e = Eng(hip, kv, P)
        m = e.m
        out = []
        m.prefill_ragged([tokens(9, 2 * P + 3), [], [], []])
        m.step(None)
        snap(e, out)
        extra = None
        if checkpoint:
            free = m.free_pages()
            h = m.park(0, keep=True)
            assert m.free_pages() == free and m.positions()[0] == 2 * P + 4  # a checkpoint takes nothing
            m.release(1), m.release(2)
            m.unpark(h, 1)
            m.unpark(h, 2)
            assert m.free_pages() == free + 2 - 2 * 3  # slots 1 and 2 held one page each
            p0, p1, p2 = (set(e.pages(b)) for b in range(3))
            assert len(p1) == len(p2) == 3 and not (p0 & p1 or p0 & p2 or p1 & p2)
            assert same_kv(e.kv_rows(1), e.kv_rows(0)) and same_kv(e.kv_rows(2), e.kv_rows(0))
            ids = e.next_ids()
            assert ids[0] == ids[1] == ids[2]
            h.free()
        snap(e, out)
        for _ in range(3):
            nxt = m.step(None)
            snap(e, out)
            if checkpoint:  # the two copies and the source continue alike (greedy)
                lg = m.logits()
                assert nxt[0] == nxt[1] == nxt[2]
                assert np.array_equal(lg[0], lg[1]) and np.array_equal(lg[0], lg[2])
                extra = True
        e.close()
        assert extra or not checkpoint
        for s in out:
            s["pos"] = s["pos"][:1]  # the other slots differ between the runs by design
        return out

    assert_same_snaps(run(False), run(True), (kv, P))


# ---------------------------------------------------------------- 4. shared pages
@pytest.mark.parametrize("pool", POOLS, ids=_id)
def test_parking_a_fork(hip, pool):
    kv, P = pool

    def run(park):
        e = Eng(hip, kv, P)
        m, bm = e.m, e.bm
        out = []
        m.prefill_ragged([tokens(11, 2 * P + 5), [], [], []])
        free = m.free_pages()
        m.fork(0, 1, P + 3)  # one full page shared, the partly filled one copied
        assert bm.shared_pages() == 1 and m.free_pages() == free - 1
        kv1 = e.kv_rows(1)
        if park:
            h = m.park(1)
            assert bm.shared_pages() == 0 and m.free_pages() == free and h.tokens == P + 3
        else:
            m.release(1)
        snap(e, out)
        for _ in range(2):
            m.step(None)
            snap(e, out)
        if park:
            m.release(1)  # the two steps fed it from position 0
            free1 = m.free_pages()
            m.unpark(h, 1)
            assert bm.shared_pages() == 0 and m.free_pages() == free1 - 2
            assert not set(e.pages(1)) & set(e.pages(0))
            assert same_kv(e.kv_rows(1), kv1)
            h.free()
        m.step(None)
        snap(e, out)
        e.close()
        for s in out:
            s["pos"] = s["pos"][:1]
        return out

    assert_same_snaps(run(False), run(True), (kv, P))


# ---------------------------------------------------------------- 5. processors on
def _processors_on(m):
    m.set_processors(True)
    m.set_penalties(0, repetition=1.4, presence=0.3, frequency=0.2, from_pos=1)
    m.set_logit_bias(0, [5, 11], [2.0, -np.inf])


def _processor_reads(e):
    m = e.m
    return dict(history=m.history(0), counts=m.token_counts(0), processed=m.processed_logits()[0].copy())


@pytest.mark.parametrize("mode", [0, 2], ids=["greedy", "filtered"])
@pytest.mark.parametrize("pool", POOLS, ids=_id)
def test_processors_travel(hip, pool, mode):
    kv, P = pool
    n = P + 1
    want, _, _ = same_slot_script(hip, kv, P, n, mode, True, park=False, setup=_processors_on, extra=_processor_reads)
    got, _, _ = same_slot_script(hip, kv, P, n, mode, True, park=True, setup=_processors_on, extra=_processor_reads)
    assert_same_snaps(want, got, (kv, P, mode))
    for i, (x, y) in enumerate(zip(want, got)):
        assert np.array_equal(x["history"], y["history"]) and len(x["history"]) == x["pos"][0], i
        assert np.array_equal(x["counts"], y["counts"]), i
        assert np.array_equal(x["processed"].view(np.uint32), y["processed"].view(np.uint32)), i
    assert want[-1]["counts"].sum() == n + 7 - 1  # the window starts at position 1
    assert np.isneginf(want[-1]["processed"][11])


def test_history_is_required_where_processors_are_on(hip):
    a, b = Eng(hip), Eng(hip)
    a.m.prefill_ragged([tokens(3, 20), [], [], []])
    h = a.m.park(0)
    b.m.set_processors(True)
    before = b.state()
    with pytest.raises(RuntimeError):
        b.m.unpark(h, 0)
    assert b.state() == before
    a.m.unpark(h, 0)  # the engine it came from takes it
    h.free()
    a.close()
    b.close()


# ---------------------------------------------------------------- 6. log-probabilities
@pytest.mark.parametrize("pool", [POOLS[0], POOLS[3], POOLS[4]], ids=_id)
def test_logprob_readbacks_travel(hip, pool):
    kv, P = pool
    e = Eng(hip, kv, P)
    m = e.m
    m.set_logprobs(True)
    m.set_top_logprobs(5)
    m.prefill_ragged([tokens(13, P + 2), tokens(14, 3), [], []])
    m.step(None)
    lp, (ids, lps) = m.logprobs(), m.top_logprobs()
    assert np.isfinite(lp[0]) and lp[0] < 0 and len(set(ids[0].tolist())) == 5
    h = m.park(0)
    m.prefill_ragged([[], tokens(15, 2 * P), [], []])  # slot 1 picks again: its rows change, slot 0's are gone
    for seq in (0, 3):
        if seq == 3:
            m.release(3)
        m.unpark(h, seq)
        lp2, (ids2, lps2) = m.logprobs(), m.top_logprobs()
        assert lp2[seq].tobytes() == lp[0].tobytes()
        assert np.array_equal(ids2[seq], ids[0]) and np.array_equal(lps2[seq].view(np.uint32), lps[0].view(np.uint32))
    h.free()
    e.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals_change_nothing(hip):
    P = 16
    e = Eng(hip, "f32", P, pages=8)
    m = e.m
    m.prefill_ragged([tokens(17, 40), [], [], []])  # 3 pages
    h = m.park(0, keep=True)
    m.prefill_ragged([[], tokens(18, 35), [], []])  # 3 more: 2 free, one short of the 3 the handle needs
    assert m.free_pages() == 2 and h.tokens == 40
    before = e.state()
    for seq in (0, 1, -1, B):  # live targets, no such slot
        with pytest.raises(RuntimeError):
            m.unpark(h, seq)
        assert e.state() == before, seq
    with pytest.raises(RuntimeError):
        m.unpark(h, 2)  # one page short
    assert e.state() == before
    for seq in (2, 3, -1, B):  # nothing cached, no such slot
        with pytest.raises(RuntimeError):
            m.park(seq)
        assert e.state() == before, seq
    m.release(1)
    m.unpark(h, 2)  # now it fits: 5 free, 3 taken
    assert m.free_pages() == 2 and m.positions().tolist() == [40, 0, 40, 0]
    h.free()
    e.close()


def test_other_geometries_are_refused(hip):
    src = {"f32": Eng(hip, "f32", 16), "fp8": Eng(hip, "fp8", 16)}
    handles = {}
    for kv, e in src.items():
        e.m.prefill_ragged([tokens(19, 21), [], [], []])
        handles[kv] = e.m.park(0, keep=True)
    other_v = dict(SMALL, V=992)
    targets = [("f32", Eng(hip, "f32", 64)),            # another page size
               ("f32", Eng(hip, "bf16", 16)),           # another dtype
               ("fp8", Eng(hip, "fp8", 16, scale_seed=1)),  # other scales
               ("f32", Eng(hip, "f32", 16, cfgd=other_v))]  # another vocabulary
    for kv, t in targets:
        before = t.state()
        with pytest.raises(RuntimeError):
            t.m.unpark(handles[kv], 0)
        assert t.state() == before
        t.close()
    for kv in src:  # an engine of the same geometry (fp8: the same scales) takes the other's handle
        twin = Eng(hip, kv, 16)
        twin.m.unpark(handles[kv], 3)
        assert same_kv(twin.kv_rows(3), src[kv].kv_rows(0))
        assert np.array_equal(twin.m.logits()[3].view(np.uint32), src[kv].m.logits()[0].view(np.uint32))
        assert twin.m.step(None)[3] == src[kv].m.step(None)[0]
        twin.close()
    for kv, e in src.items():
        handles[kv].free()
        e.close()


# ---------------------------------------------------------------- 8. pool accounting
@pytest.mark.parametrize("pool", POOLS, ids=_id)
def test_pool_accounting(hip, pool):
    kv, P = pool
    e = Eng(hip, kv, P)
    m = e.m
    L = hip.lib()
    shape = e.pool_shape()
    for n in (1, P, P + 1, 3 * P - 1):
        m.prefill_ragged([tokens(n, n), [], [], []])
        pages = -(-n // P)
        free = m.free_pages()
        h = m.park(0, keep=True)
        assert m.free_pages() == free
        assert h.tokens == n == L.gpt2_parked_tokens(h.h)
        assert h.bytes == hip.park_bytes(shape, pages) == SMALL["L"] * pages * 2 * SMALL["C"] * P * pm.ELEM_BYTES[KV[kv]]
        h.free()
        h = m.park(0)
        assert m.free_pages() == free + pages and m.positions()[0] == 0 and h.tokens == n and h.bytes > 0
        h.free()
        h.free()  # idempotent in the binding
    L.gpt2_parked_free(None)
    assert L.gpt2_parked_tokens(None) == 0 and L.gpt2_parked_bytes(None) == 0
    e.close()
