"""Prefix sharing (gpt2_decode_fork): a slot forks another slot's cached prefix,
sharing its full pages and copying only the partly filled one
(hpa_pool_copy_pages), then the two diverge.

Bars as tests/test_gpu_serving.py, whose SMALL config this file uses: logits
within 2e-4 of one oracle PagedDecoder per sequence fed that sequence's full
token history (a fork's history is the source's prefix plus its own tokens),
greedy ids equal where the oracle's top-2 margin exceeds 1e-3.  What a fork
shares or copies is compared bit for bit.
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import synth

pytestmark = pytest.mark.gpu
SMALL = dict(maxT=256, V=1000, L=2, NH=2, C=128)
LOGIT_TOL = 2e-4
TIE_MARGIN = 1e-3


class Request:
    """one sequence in the oracle: a B = 1 paged decoder fed token by token"""

    def __init__(self, params, c, P, seed):
        self.o = oc.PagedDecoder(params, c, 1, P, SMALL["maxT"], page_seed=seed)

    def feed(self, toks):
        for t in toks:
            nxt, lg = self.o.step(np.array([t], np.int32))
        return int(nxt[0]), lg[0]

    def pos(self):
        return self.o.pos(0)

    def close(self):
        self.o.close()


class Forks:
    """the engine's slots, each next to its token history and an oracle Request
    that was fed exactly that history"""

    def __init__(self, hip, B, P=16, seed=1, bm=None, kv_dtype=0, oracle=True):
        self.params = synth.params(SMALL, seed=seed)
        self.c = oc.cfg(SMALL["maxT"], SMALL["V"], SMALL["L"], SMALL["NH"], SMALL["C"])
        self.model = hip.Model(SMALL, params=self.params)
        if bm is not None:
            self.model.set_manager(bm)
        self.model.decode_init(B, P, SMALL["maxT"], kv_dtype=kv_dtype)
        self.B, self.P, self.oracle = B, P, oracle
        self.rng = np.random.default_rng(seed)
        self.reqs = [None] * B
        self.hist = [[] for _ in range(B)]
        self.cur = [0] * B  # the oracle's next id per slot
        self.worst = 0.0
        self.n_req = 0

    def tokens(self, n):
        return [int(t) for t in self.rng.integers(0, SMALL["V"], n)]

    def _request(self):
        self.n_req += 1
        return Request(self.params, self.c, self.P, seed=100 + self.n_req) if self.oracle else None

    def admit(self, b, n):
        assert self.reqs[b] is None and not self.hist[b]
        self.reqs[b] = self._request()
        return self.tokens(n)

    def fork(self, src, dst, n=-1):
        """engine fork + an oracle of its own for dst, fed the shared prefix"""
        self.model.fork(src, dst, n)
        n = len(self.hist[src]) if n == -1 else n
        self.hist[dst] = self.hist[src][:n]
        self.reqs[dst] = self._request()
        if self.oracle:
            self.cur[dst], _ = self.reqs[dst].feed(self.hist[dst])

    def drop(self, b, release=True):
        if release:
            self.model.release(b)
        if self.reqs[b] is not None:
            self.reqs[b].close()
        self.reqs[b], self.hist[b] = None, []

    def _check(self, b, toks, g_next, logits):
        self.hist[b] += [int(t) for t in toks]
        o_next, o_logits = self.reqs[b].feed(toks)
        diff = float(np.abs(logits[b] - o_logits).max())
        self.worst = max(self.worst, diff)
        assert diff <= LOGIT_TOL, (b, diff)
        s = np.sort(o_logits)
        if s[-1] - s[-2] > TIE_MARGIN:
            assert g_next[b] == o_next, (b, g_next[b], o_next)
        self.cur[b] = o_next

    def run(self, batch):
        """batch: slot -> tokens; one ragged call for all of them"""
        g_next = self.model.prefill_ragged([batch.get(b, []) for b in range(self.B)])
        logits = self.model.logits()
        for b, toks in batch.items():
            self._check(b, toks, g_next, logits)
        self.check_positions()

    def decode(self, toks):
        """one plain decode step of every slot (all live) with these tokens"""
        g_next = self.model.step(np.array(toks, np.int32))
        logits = self.model.logits()
        for b in range(self.B):
            self._check(b, [toks[b]], g_next, logits)
        self.check_positions()

    def check_positions(self):
        pos = self.model.positions()
        for b, r in enumerate(self.reqs):
            if r is not None:
                assert pos[b] == len(self.hist[b]) == r.pos(), (b, pos[b], len(self.hist[b]), r.pos())

    def read_kv(self, b, n):
        return [self.model.read_kv(l, b, n) for l in range(SMALL["L"])]

    def close(self):
        for r in self.reqs:
            if r is not None:
                r.close()
        self.model.close()


def same_kv(a, b):
    return all(np.array_equal(ka, kb) and np.array_equal(va, vb) for (ka, va), (kb, vb) in zip(a, b))


# ---------------------------------------------------------------- the copy kernel
def pool_bytes(hip, pool):
    out = np.empty(pool.s.bytes, np.uint8)
    hip.check(hip.lib().hpa_synchronize())
    hip.check(hip.lib().hpa_memcpy(out.ctypes.data, pool.s.base, out.nbytes), "pool download")
    return out.reshape(pool.s.num_layers, pool.s.num_pages, -1)


@pytest.mark.parametrize("dtype,P,NH", [("f32", 16, 2), ("bf16", 8, 2), ("fp8", 16, 2),
                                        ("f32", 16, 3)])  # 24 KiB pages: two workgroups per page, the second half full
def test_copy_pages(hip, dtype, P, NH):
    """destination pages equal their sources byte for byte in both layers, every
    other byte of the pool is unchanged; bad page lists launch nothing"""
    dt = dict(f32=hip.HPA_F32, bf16=hip.HPA_BF16, fp8=hip.HPA_FP8)[dtype]
    layers, pages = 2, 8
    pool = hip.Pool(layers, NH, P, pages, dtype=dt)
    bt = np.arange(pages, dtype=np.int32).reshape(2, 4)
    d_bt = hip.DeviceBuffer.from_array(bt)
    hip.check(hip.lib().hpa_pool_fill_random(pool.ref, d_bt.ptr, 4, 2, 4 * P, 4321))
    before = pool_bytes(hip, pool)
    assert before.shape[2] == 2 * NH * P * 64 * pool.s.elem_bytes
    for l in range(layers):  # the fill gave every page its own bytes
        assert len({before[l, p].tobytes() for p in range(pages)}) == pages
    pool.copy_pages([1, 5], [2, 7])
    pool.copy_pages([0], [3])
    after = pool_bytes(hip, pool)
    want = before.copy()
    want[:, 2], want[:, 7], want[:, 3] = before[:, 1], before[:, 5], before[:, 0]
    assert np.array_equal(after, want)
    for src, dst in [([], []),                                  # n = 0
                     (list(range(65)), list(range(65, 130))),   # n = 65
                     ([1], [pages]), ([-1], [2]), ([pages], [2]),  # out of range
                     ([4], [4]),                                # src == dst
                     ([1, 2], [2, 3]),                          # page 2 both a destination and a source
                     ([1, 4], [6, 6])]:                         # one destination twice
        with pytest.raises(RuntimeError):
            pool.copy_pages(src, dst)
    assert np.array_equal(pool_bytes(hip, pool), want)
    d_bt.free()
    pool.destroy()


# ---------------------------------------------------------------- the engine call
@pytest.mark.parametrize("graph", [False, True])
def test_fork_then_diverge(hip, graph):
    """37 tokens = 2 full pages + 5: each fork shares the two and copies the
    third; 14 steps with different tokens per slot cross the page boundary at
    48; nobody writes into the source's prefix"""
    s = Forks(hip, B=3, P=16, seed=11)
    s.model.set_graph(graph)
    s.run({0: s.admit(0, 37)})
    free = s.model.free_pages()
    s.fork(0, 1)
    assert s.model.free_pages() == free - 1
    s.fork(0, 2)
    assert s.model.free_pages() == free - 2
    assert list(s.model.positions()) == [37, 37, 37]
    src_kv = s.read_kv(0, 37)
    assert any(np.abs(k).max() > 0 for k, _ in src_kv)
    assert same_kv(s.read_kv(1, 37), src_kv) and same_kv(s.read_kv(2, 37), src_kv)
    for _ in range(14):
        s.decode([s.cur[0]] + s.tokens(2))
    assert list(s.model.positions()) == [51, 51, 51]
    assert same_kv(s.read_kv(0, 37), src_kv)
    assert same_kv(s.read_kv(1, 37), src_kv) and same_kv(s.read_kv(2, 37), src_kv)
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()


def test_fork_boundary_and_prefix(hip):
    """a fork at a page boundary copies nothing; a fork of a shorter prefix takes
    one page and continues with tokens of its own"""
    s = Forks(hip, B=3, P=16, seed=12)
    s.run({0: s.admit(0, 37)})
    free = s.model.free_pages()
    s.fork(0, 1, 32)
    assert s.model.free_pages() == free and s.model.positions()[1] == 32
    s.fork(0, 2, 20)
    assert s.model.free_pages() == free - 1 and s.model.positions()[2] == 20
    src_kv = s.read_kv(0, 37)
    assert same_kv(s.read_kv(1, 32), [(k[:32], v[:32]) for k, v in src_kv])
    assert same_kv(s.read_kv(2, 20), [(k[:20], v[:20]) for k, v in src_kv])
    s.run({0: [s.cur[0]], 2: s.tokens(9)})      # slot 2: positions 20..28 of its own page
    s.run({0: [s.cur[0]], 1: s.tokens(1)})      # slot 1: position 32, the first slot of a page of its own
    assert s.model.free_pages() == free - 2
    for _ in range(2):
        s.decode([s.cur[0]] + s.tokens(2))
    assert same_kv(s.read_kv(0, 37), src_kv)
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()


@pytest.mark.parametrize("kv,P", [("f32", 16), ("bf16", 8), ("fp8", 16)])
def test_fork_inherits_next_id(hip, kv, P):
    """after fork(0, 1) a device-fed step continues both: the same next id and
    bit-equal logits rows (the two rows hold the same K/V bits, and a row of
    one launch does not depend on its index)"""
    dt = dict(f32=hip.HPA_F32, bf16=hip.HPA_BF16, fp8=hip.HPA_FP8)[kv]
    s = Forks(hip, B=2, P=P, seed=13, kv_dtype=dt, oracle=kv == "f32")
    toks = s.admit(0, 37)
    fed = int(s.model.prefill_ragged([toks, []])[0])  # the id the device feeds back next
    s.hist[0] = toks
    if s.oracle:
        s.reqs[0].feed(toks)
    s.fork(0, 1)
    assert same_kv(s.read_kv(1, 37), s.read_kv(0, 37))
    for _ in range(2):
        nxt = s.model.step(None)
        lg = s.model.logits()
        assert nxt[1] == nxt[0]
        assert np.array_equal(lg[1], lg[0])
        assert np.isfinite(lg).all() and np.abs(lg[0]).max() > 0
        if s.oracle:  # the continued rows are right, not only equal
            _, o_logits = s.reqs[0].feed([fed])
            assert float(np.abs(lg[0] - o_logits).max()) <= LOGIT_TOL
        fed = int(nxt[0])
    assert list(s.model.positions()) == [39, 39]
    assert same_kv(s.read_kv(1, 39), s.read_kv(0, 39))
    s.close()


def test_release_order_on_the_engine(hip):
    """the source goes first: the fork keeps the shared pages and decodes on;
    releasing everything returns every page"""
    s = Forks(hip, B=2, P=16, seed=14)
    capacity = s.model.free_pages()
    assert capacity == 2 * (SMALL["maxT"] // 16)
    s.run({0: s.admit(0, 37)})
    s.fork(0, 1)
    assert s.model.free_pages() == capacity - 4
    s.drop(0)
    assert s.model.free_pages() == capacity - 3 and s.model.positions()[0] == 0
    for _ in range(3):
        s.run({1: [s.cur[1]]})
    assert s.worst <= LOGIT_TOL, s.worst
    s.drop(1)
    assert s.model.free_pages() == capacity
    s.close()


def test_rewind_into_a_shared_page_copies_it(hip):
    """set_positions rewinds the fork into a page it shares: its next append
    lands in a private copy, the source's bytes stay"""
    s = Forks(hip, B=2, P=16, seed=15)
    s.run({0: s.admit(0, 37)})
    s.fork(0, 1)
    src_kv = s.read_kv(0, 37)
    free = s.model.free_pages()
    s.model.set_positions([37, 10])
    s.reqs[1].close()
    s.hist[1] = s.hist[0][:10]
    s.reqs[1] = s._request()
    s.reqs[1].feed(s.hist[1])
    s.decode([s.cur[0], s.tokens(1)[0]])
    assert s.model.free_pages() == free - 1
    assert same_kv(s.read_kv(0, 37), src_kv)
    assert same_kv(s.read_kv(1, 10), [(k[:10], v[:10]) for k, v in src_kv])
    s.decode([s.cur[0], s.cur[1]])  # the page is its own now: no further copy
    assert s.model.free_pages() == free - 1
    assert same_kv(s.read_kv(0, 37), src_kv)
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()


def test_rewind_then_prefill_and_reserve(hip):
    """the guard covers every page an append lands in: a ragged prefill over
    two shared pages copies both, and reserve() makes the pages up to its
    context private before the steps run"""
    bm = hip.BlockManager(SMALL["C"], max_prompts=3, max_blocks=48, block_size=16, max_blocks_per_prompt=16)
    s = Forks(hip, B=3, P=16, seed=18, bm=bm)
    s.run({0: s.admit(0, 37)})
    s.fork(0, 1)
    src_kv = s.read_kv(0, 37)
    free = bm.free_pages()

    def rewind(b, n, pos):
        s.model.set_positions(pos)
        s.reqs[b].close()
        s.hist[b] = s.hist[0][:n]
        s.reqs[b] = s._request()
        s.reqs[b].feed(s.hist[b])

    rewind(1, 10, [37, 10, 0])
    s.run({1: s.tokens(30)})  # positions 10..39: shared pages 0 and 1, then its own third page
    assert bm.free_pages() == free - 2 and bm.shared_pages() == 0
    assert same_kv(s.read_kv(0, 37), src_kv)
    s.fork(0, 2)
    assert bm.shared_pages() == 2 and bm.free_pages() == free - 3
    rewind(2, 5, [37, 40, 5])
    s.model.reserve(64)  # slot 2: two shared pages copied + a fourth page; slots 0 and 1: a fourth page each
    assert bm.shared_pages() == 0 and bm.free_pages() == free - 3 - 5
    assert [len(bm.pages(b)) for b in range(3)] == [4, 4, 4]
    assert same_kv(s.read_kv(2, 5), [(k[:5], v[:5]) for k, v in src_kv])
    for _ in range(2):
        s.decode([s.cur[0], s.cur[1], s.tokens(1)[0]])
    assert bm.free_pages() == free - 8
    assert same_kv(s.read_kv(0, 37), src_kv)
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()
    bm.close()


def test_eviction_keeps_the_fork_alive(hip):
    """a caller's manager of 6 pages: evicting the source (for its private tail
    page, the LRU page with one holder) leaves the shared pages to the fork"""
    bm = hip.BlockManager(SMALL["C"], max_prompts=3, max_blocks=6, block_size=16, max_blocks_per_prompt=16)
    s = Forks(hip, B=3, P=16, seed=16, bm=bm)
    s.run({0: s.admit(0, 40)})
    s.fork(0, 1)
    assert bm.pages(0) == [0, 1, 2] and bm.pages(1) == [0, 1, 3] and bm.shared_pages() == 2
    s.run({2: s.admit(2, 31)})
    assert bm.free_pages() == 0 and not s.model.evicted().any()
    s.reqs[0].close()
    s.reqs[0], s.hist[0] = None, []  # about to be paged out
    s.run({2: [s.cur[2]] + s.tokens(1)})  # positions 31, 32: a third page
    assert list(s.model.evicted()) == [True, False, False]
    assert s.model.positions()[0] == 0
    assert bm.pages(0) == [] and bm.pages(1) == [0, 1, 3] and bm.pages(2) == [4, 5, 2]
    assert bm.shared_pages() == 0 and [bm.refs(p) for p in (0, 1)] == [1, 1]
    s.run({1: [s.cur[1]], 2: [s.cur[2]]})
    s.run({1: [s.cur[1]], 2: [s.cur[2]]})
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()
    bm.close()


def test_fork_refusals(hip):
    s = Forks(hip, B=3, P=16, seed=17, oracle=False)
    s.model.prefill_ragged([s.tokens(37), s.tokens(5), []])
    pos, free = list(s.model.positions()), s.model.free_pages()
    for src, dst, n in [(0, 1, -1),            # slot 1 is live
                        (0, 2, 0), (0, 2, 38), (0, 2, -2),
                        (2, 1, -1),            # nothing cached in the source (and a live destination)
                        (0, 0, -1), (2, 2, 1),  # src == dst
                        (0, 3, -1), (-1, 2, 1), (3, 2, 1)]:
        with pytest.raises(RuntimeError):
            s.model.fork(src, dst, n)
        assert list(s.model.positions()) == pos and s.model.free_pages() == free, (src, dst, n)
    s.model.fork(0, 2)
    assert s.model.free_pages() == free - 1
    with pytest.raises(RuntimeError):
        s.model.fill_random(20)  # it would overwrite pages two slots hold
    assert list(s.model.positions()) == [37, 5, 37]
    s.model.release(2)
    s.model.fill_random(20)  # nothing shared any more
    s.close()
