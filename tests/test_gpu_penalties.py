"""Logit processors in the decode engine: repetition / presence / frequency
penalties over the fed tokens and a logit bias, per sequence, before every
pick (include/paged_infer.h states the contract).

The test keeps its own books: the tokens it knows were fed to every sequence.
Each check rebuilds the counts from them, computes the float64 reference from
m.logits() (logit_ref64.process) and asserts
  - m.processed_logits() within tol = 2^-21 S per element (-inf where the
    reference is -inf);
  - the picked id's reference value within 2 tol of the reference row maximum
    (greedy), or the sampler's criterion on m.processed_logits() (modes 1, 2).
No case is skipped.
"""
import numpy as np
import pytest

import logit_ref64 as lr
import oracle_ctypes as oc
import sample_ref64 as sr
import score_ref64 as scr
import synth

pytestmark = pytest.mark.gpu

SMALL = dict(maxT=128, V=1000, L=2, NH=2, C=128)
V = SMALL["V"]
B, PAGE = 6, 16
NEUTRAL = dict(r=1.0, p=0.0, f=0.0, frm=0, ids=[], vals=[])


class Book:
    """an engine with processors on, next to the test's own record of what was fed"""

    def __init__(self, hip, settings, B=B, graph=True, bm=None, enable=True):
        self.m = hip.Model(SMALL, params=synth.params(SMALL, seed=3))
        if bm is not None:
            self.m.set_manager(bm)
        self.m.decode_init(B, PAGE, SMALL["maxT"])
        self.m.set_graph(graph)
        self.B = B
        self.hist = [[] for _ in range(B)]
        self.pending = np.zeros(B, np.int32)
        self.set = [dict(NEUTRAL) for _ in range(B)]
        if enable:
            self.m.set_processors(True)
        for b, s in enumerate(settings):
            self.configure(b, **s)

    def configure(self, b, **kw):
        s = self.set[b]
        s.update(kw)
        self.m.set_penalties(b, s["r"], s["p"], s["f"], s["frm"])
        self.m.set_logit_bias(b, s["ids"], s["vals"])

    def reference(self, b, raw):
        s = self.set[b]
        c = lr.counts_from(self.hist[b], s["frm"], len(self.hist[b]), V)
        return lr.process(raw[b], c, s["r"], s["p"], s["f"], s["ids"], s["vals"])

    def check(self, ids, rows=None, greedy=True):
        """processed rows against the reference from m.logits(); greedy ids"""
        raw, proc = self.m.logits(), self.m.processed_logits()
        worst = 0.0
        for b in (range(self.B) if rows is None else rows):
            y, tol = self.reference(b, raw)
            worst = max(worst, lr.assert_close(proc[b], y, tol, ("row", b)))
            if greedy:
                w = lr.winner(y)
                assert y[w] - y[ids[b]] <= 2.0 * max(tol[w], tol[ids[b]]), (b, int(ids[b]), w, y[ids[b]], y[w])
            assert np.isfinite(y[ids[b]]), ("a banned id was picked", b, int(ids[b]))
        assert np.array_equal(self.m.positions(), [len(h) for h in self.hist])
        return worst

    def prefill(self, seqs):
        ids = self.m.prefill_ragged(seqs)
        for b, t in enumerate(seqs):
            self.hist[b] += [int(x) for x in t]
            if len(t):
                self.pending[b] = ids[b]
        return ids

    def step(self, tokens=None):
        """tokens None: the pending ids are fed back on the device"""
        fed = self.pending.copy() if tokens is None else np.asarray(tokens, np.int32)
        ids = self.m.step(None if tokens is None else fed)
        for b in range(self.B):
            self.hist[b].append(int(fed[b]))
        self.pending = ids.copy()
        return ids

    def check_readbacks(self, rows=None):
        for b in (range(self.B) if rows is None else rows):
            s = self.set[b]
            assert self.m.history(b).tolist() == self.hist[b], b
            want = lr.counts_from(self.hist[b], s["frm"], len(self.hist[b]), V)
            assert np.array_equal(self.m.token_counts(b), want), b

    def close(self):
        self.m.close()


def _prompts(rng, lens):
    # a small alphabet so that prompts repeat tokens and the counts pass 1
    return [rng.integers(0, 40, n).astype(np.int32).tolist() for n in lens]


def _settings(lens):
    rng = np.random.default_rng(5)
    ban = [int(t) for t in rng.permutation(V) if t not in (7, 8)][:60]  # 7 and 8 carry row 4's finite biases
    return [dict(NEUTRAL),
            dict(r=1.3),
            dict(p=0.6, f=0.2, frm=lens[2]),  # OpenAI style: generated tokens only
            dict(ids=ban, vals=[-np.inf] * 60),
            dict(r=1.2, p=0.4, f=0.1, frm=3, ids=ban[:20] + [7, 8], vals=[-np.inf] * 20 + [2.5, -1.5]),
            dict(r=0.8, f=-0.05)]  # below 1 / negative: favours what was said


def test_greedy_steps_with_per_row_settings(hip):
    lens = [5, 9, 12, 7, 16, 3]
    bk = Book(hip, _settings(lens))
    plain = Book(hip, [], enable=False)  # never enables processors; fed the same tokens
    assert plain.m.processed_logits() is None and not plain.m.processors() and bk.m.processors()
    prompts = _prompts(np.random.default_rng(1), lens)
    ids = bk.prefill(prompts)
    pids = plain.prefill(prompts)
    worst = bk.check(ids)
    assert ids[0] == pids[0]
    for s in range(24):
        fed = bk.pending.copy()
        ids = bk.step(None)  # fed back on the device under the captured graph
        worst = max(worst, bk.check(ids))
        pids = plain.step(fed)
        # the neutral row: ids, raw logits and processed logits are the plain engine's bits
        assert ids[0] == pids[0], (s, ids[0], pids[0])
        lg0 = bk.m.logits()[0]
        assert lg0.tobytes() == plain.m.logits()[0].tobytes()
        assert bk.m.processed_logits()[0].tobytes() == lg0.tobytes()
    banned = set(bk.set[3]["ids"])
    assert not banned & set(bk.hist[3][lens[3]:])
    bk.check_readbacks()
    print(f"[penalties] 24 greedy steps: largest error / tol {worst:.3f}")
    bk.close()
    plain.close()


def test_settings_change_under_graph_replay(hip):
    lens = [4, 4, 4, 4, 4, 4]
    bk = Book(hip, _settings(lens))
    ids = bk.prefill(_prompts(np.random.default_rng(2), lens))
    bk.check(ids)
    for s in range(24):
        if s == 8:  # from the next step on, without recapture: the kernel reads device memory
            bk.configure(0, r=1.7, p=0.3)
            bk.configure(1, r=1.0)
            bk.configure(3, ids=[int(ids[3]), 11], vals=[-np.inf, 1.0])
            bk.configure(2, frm=2)  # a window change recounts
        if s == 16:  # and back
            bk.configure(0, r=1.0, p=0.0)
            bk.configure(1, r=1.3)
            bk.configure(3, ids=[], vals=[])
            bk.configure(2, frm=4)
        ids = bk.step(None)
        bk.check(ids)
        if s in (8, 16):
            bk.check_readbacks()
    assert bk.m.penalties(1) == pytest.approx((1.3, 0.0, 0.0, 0))
    assert bk.m.logit_bias(3)[0].size == 0
    bk.close()


def test_history_and_count_readbacks(hip):
    bk = Book(hip, [dict(NEUTRAL), dict(frm=2), dict(frm=100), dict(r=1.5), dict(frm=5), dict(NEUTRAL)])
    rng = np.random.default_rng(3)
    seqs = _prompts(rng, [6, 10, 3, 0, 17, 1])  # row 3 empty: nothing recorded, nothing picked
    ids = bk.prefill(seqs)
    assert bk.m.history(3).size == 0 and bk.m.token_counts(3).sum() == 0
    bk.check(ids, rows=[0, 1, 2, 4, 5])
    bk.check_readbacks()
    proc3 = bk.m.processed_logits()[3].copy()
    ids2 = bk.prefill([[1, 1], [], [2], [], [], [9, 9, 9]])  # rows left alone keep their processed row and next id
    assert np.array_equal(ids2[[1, 3, 4]], ids[[1, 3, 4]])
    assert bk.m.processed_logits()[3].tobytes() == proc3.tobytes()
    bk.check(ids2, rows=[0, 2, 5])
    bk.check_readbacks()
    tok = rng.integers(0, 40, B).astype(np.int32)
    bk.check(bk.step(tok))  # host-fed
    bk.check_readbacks()
    for _ in range(3):
        bk.check(bk.step(None))  # device-fed
    bk.check_readbacks()
    bk.configure(1, frm=0)  # the window moves: a recount from the history
    bk.configure(4, frm=12)
    bk.check_readbacks()
    bk.check(bk.step(None))
    bk.close()


def test_fork_full_and_partial_prefix(hip):
    bk = Book(hip, [dict(r=1.3), dict(p=0.5, f=0.1), dict(NEUTRAL), dict(NEUTRAL), dict(f=0.3, frm=4),
                    dict(r=1.4, frm=3)])
    rng = np.random.default_rng(4)
    seqs = _prompts(rng, [37, 29, 5, 2, 0, 0])
    ids = bk.prefill(seqs)
    bk.check(ids, rows=[0, 1, 2, 3])
    bk.m.fork(0, 4)  # the whole prefix, the pending id with it
    bk.hist[4] = list(bk.hist[0])
    bk.pending[4] = bk.pending[0]
    bk.m.fork(1, 5, 21)  # a partial prefix: no multiple of 16, the page size
    bk.hist[5] = bk.hist[1][:21]
    bk.check_readbacks()  # dst: the prefix's history, counted over dst's own window
    assert bk.m.penalties(4) == pytest.approx((1.0, 0.0, 0.3, 4)) and bk.m.penalties(5)[0] == pytest.approx(1.4)
    tok = bk.pending.copy()
    tok[5] = bk.hist[1][21]  # the partial fork continues with a token of its own
    bk.check(bk.step(tok))
    for _ in range(4):
        bk.check(bk.step(None))
    bk.check_readbacks()
    bk.close()


def test_release_and_readmission_count_only_the_new_prompt(hip):
    bk = Book(hip, [dict(r=1.3, p=0.2)] * B)
    rng = np.random.default_rng(6)
    bk.check(bk.prefill(_prompts(rng, [20] * B)))
    bk.check(bk.step(None))
    before = bk.m.penalties(2), bk.m.logit_bias(2)[0].tolist()
    bk.m.release(2)
    bk.hist[2] = []
    assert bk.m.token_counts(2).sum() == 0 and bk.m.history(2).size == 0
    assert (bk.m.penalties(2), bk.m.logit_bias(2)[0].tolist()) == before  # the settings stay
    new = _prompts(rng, [0, 0, 11, 0, 0, 0])
    ids = bk.prefill(new)
    bk.check(ids, rows=[2])
    bk.check_readbacks()
    assert bk.m.token_counts(2).sum() == 11
    bk.check(bk.step(None))
    bk.m.reset()  # every sequence restarts
    for b in range(B):
        assert bk.m.token_counts(b).sum() == 0 and bk.m.history(b).size == 0
    bk.close()


def test_lru_eviction_zeroes_the_evicted_slots_counts(hip):
    """a pool of 5 pages for 2 sequences (test_gpu_serving.py): growing
    sequence 1 evicts sequence 0 whole, which restarts at position 0"""
    bm = hip.BlockManager(SMALL["C"], max_prompts=2, max_blocks=5, block_size=16, max_blocks_per_prompt=16)
    bk = Book(hip, [dict(r=1.3, f=0.1)] * 2, B=2, bm=bm)
    rng = np.random.default_rng(7)
    bk.check(bk.prefill(_prompts(rng, [40, 31])))  # 3 + 2 pages: the pool is full
    bk.check(bk.step(None))  # sequence 1 writes position 31: no eviction yet
    fed = bk.pending.copy()
    ids = bk.m.step(None)  # sequence 1 needs a third page: sequence 0 (LRU) is evicted and restarts
    assert bk.m.evicted().tolist() == [True, False]
    bk.hist[0] = [int(fed[0])]
    bk.hist[1].append(int(fed[1]))
    bk.pending = ids.copy()
    bk.check(ids)
    bk.check_readbacks()
    assert bk.m.token_counts(0).sum() == 1
    bk.close()
    bm.close()


def test_rewind_recounts_and_forward_is_refused(hip):
    bk = Book(hip, [dict(r=1.3), dict(f=0.2, frm=6), dict(p=0.5), dict(NEUTRAL), dict(NEUTRAL), dict(r=1.1)])
    rng = np.random.default_rng(8)
    bk.check(bk.prefill(_prompts(rng, [20, 20, 20, 20, 20, 20])))
    for _ in range(2):
        bk.check(bk.step(None))
    pos = bk.m.positions()
    with pytest.raises(RuntimeError):  # above the recorded history
        bk.m.set_positions(pos + np.array([0, 0, 1, 0, 0, 0], np.int32))
    assert np.array_equal(bk.m.positions(), pos)
    bk.check_readbacks()
    new = pos - np.array([5, 17, 0, 22, 1, 0], np.int32)  # row 1 to inside its window's start, row 3 to 0
    bk.m.set_positions(new)
    full = [list(h) for h in bk.hist]
    bk.hist = [h[:n] for h, n in zip(bk.hist, new)]
    bk.check_readbacks()
    tok = rng.integers(0, 40, B).astype(np.int32)
    bk.check(bk.step(tok))
    bk.check_readbacks()
    back = new + 1 + np.array([2, 0, 0, 0, 0, 0], np.int32)  # forward again inside what was recorded before
    bk.m.set_positions(back)
    bk.hist[0] = bk.hist[0] + full[0][len(bk.hist[0]):back[0]]
    bk.check_readbacks()
    bk.close()


def test_modes_1_and_2_pick_from_the_processed_rows(hip):
    lens = [6] * B
    settings = _settings(lens)
    bk = Book(hip, settings)
    params = [(0.0, 0, 1.0), (0.8, 50, 1.0), (1.0, 0, 0.9), (1.0, 0, 1.0), (1.7, 0, 1.0), (1.2, 200, 0.5)]
    for b, (t, k, p) in enumerate(params):
        bk.m.set_sampling_params(b, t, k, p)
    bk.m.set_sampling(True, seed=1337, filtered=True)
    states = [1337 + b for b in range(B)]

    def check_mode2(ids):
        bk.check(ids, greedy=False)
        proc = bk.m.processed_logits()
        for b in range(B):
            states[b], u = sr.coin(states[b])
            t, k, p = params[b]
            tol = sr.tolerance(proc[b], t) if t > 0 else 0.0
            sr.check_pick_any(proc[b], t, k, p, u, int(ids[b]), tol)

    check_mode2(bk.prefill(_prompts(np.random.default_rng(9), lens)))
    for _ in range(14):
        check_mode2(bk.step(None))
    for b in (3, 4):
        assert not set(settings[b]["ids"][:20]) & set(bk.hist[b][lens[b]:])  # the banned ids never appear
    bk.close()

    bk = Book(hip, settings)  # mode 1: the reference sampler on the processed rows
    bk.m.set_sampling(True, seed=77)
    sampler = oc.Sampler(B, seed=77)
    ids = bk.prefill(_prompts(np.random.default_rng(9), lens))
    for _ in range(12):
        bk.check(ids, greedy=False)
        want = sampler.sample(bk.m.processed_logits())
        assert np.array_equal(ids, want), (ids, want)
        ids = bk.step(None)
    assert not set(settings[3]["ids"]) & set(bk.hist[3][lens[3]:])
    bk.close()


def test_logprobs_stay_the_raw_distribution(hip):
    lens = [8] * B
    bk = Book(hip, _settings(lens))
    bk.m.set_logprobs(True)
    ids = bk.prefill(_prompts(np.random.default_rng(10), lens))
    for _ in range(6):
        bk.check(ids)
        x = bk.m.logits()
        err = np.abs(bk.m.logprobs().astype(np.float64) - scr.logprob64(x, ids))
        assert np.all(err <= scr.kernel_bound(x, ids)), err
        ids = bk.step(None)
    bk.close()


def test_refusals_change_nothing(hip):
    bk = Book(hip, [], enable=False)
    m = bk.m
    assert m.processed_logits() is None
    with pytest.raises(RuntimeError):  # the readbacks need processors on
        m.history(0)
    with pytest.raises(RuntimeError):
        m.token_counts(0)
    m.set_penalties(2, 1.5, 0.25, 0.5, 7)  # settings may be set while off
    m.set_logit_bias(2, [3, 4], [1.0, -np.inf])
    m.step(np.zeros(B, np.int32))
    with pytest.raises(RuntimeError):  # a sequence at position > 0
        m.set_processors(True)
    assert not m.processors() and m.processed_logits() is None
    m.reset()
    m.set_processors(True)
    assert m.processors() and m.processed_logits() is not None

    before = [(m.penalties(b), m.logit_bias(b)[0].tolist(), m.logit_bias(b)[1].tolist()) for b in range(B)]
    assert before[2][0] == pytest.approx((1.5, 0.25, 0.5, 7)) and before[2][1] == [3, 4]
    assert before[2][2] == [1.0, -np.inf] and before[0] == ((1.0, 0.0, 0.0, 0), [], [])
    nan, inf = float("nan"), float("inf")
    bad_pen = [dict(repetition=0.0), dict(repetition=-1.0), dict(repetition=nan), dict(repetition=inf),
               dict(presence=nan), dict(presence=inf), dict(frequency=nan), dict(frequency=-inf),
               dict(from_pos=-1), dict(from_pos=SMALL["maxT"] + 1), dict(seq=B), dict(seq=-2)]
    for kw in bad_pen:
        args = dict(seq=1, repetition=1.2, presence=0.1, frequency=0.1, from_pos=1)
        args.update(kw)
        with pytest.raises(RuntimeError):
            m.set_penalties(**args)
    bad_bias = [([V], [0.0]), ([-1], [0.0]), ([5, 5], [0.0, 1.0]), ([5], [nan]), ([5], [inf]),
                (list(range(301)), [0.0] * 301)]
    for ids, vals in bad_bias:
        with pytest.raises(RuntimeError):
            m.set_logit_bias(1, ids, vals)
    for seq in (B, -2):
        with pytest.raises(RuntimeError):
            m.set_logit_bias(seq, [1], [0.0])
    assert [(m.penalties(b), m.logit_bias(b)[0].tolist(), m.logit_bias(b)[1].tolist()) for b in range(B)] == before
    m.set_logit_bias(1, list(range(300)), [0.5] * 300)  # the cap itself is fine
    m.set_logit_bias(1, [], [])
    m.set_penalties(1, from_pos=SMALL["maxT"])

    bk.set[2].update(r=1.5, p=0.25, f=0.5, frm=7, ids=[3, 4], vals=[1.0, -np.inf])
    bk.set[1].update(frm=SMALL["maxT"])
    ids = bk.prefill(_prompts(np.random.default_rng(11), [10] * B))
    bk.check(ids)
    pos, hist0 = m.positions(), m.history(0)
    with pytest.raises(RuntimeError):
        m.fill_random(20)
    with pytest.raises(RuntimeError):
        m.verify([[1, 2]] * B)
    with pytest.raises(RuntimeError):
        m.set_positions(pos + 1)
    assert np.array_equal(m.positions(), pos) and np.array_equal(m.history(0), hist0)
    bk.check(bk.step(None))  # and the engine goes on
    bk.check_readbacks()
    m.set_processors(False)  # switching off is allowed at any position
    assert m.processed_logits() is None and not m.processors()
    with pytest.raises(RuntimeError):  # ... switching on again is not
        m.set_processors(True)
    bk.close()


def test_two_engines_give_the_same_bits(hip):
    lens = [5, 9, 12, 7, 16, 3]
    out = []
    for _ in range(2):
        bk = Book(hip, _settings(lens))
        ids = [bk.prefill(_prompts(np.random.default_rng(12), lens)).copy()]
        rows = [bk.m.processed_logits().tobytes()]
        for _ in range(8):
            ids.append(bk.step(None).copy())
            rows.append(bk.m.processed_logits().tobytes())
        out.append((np.array(ids).tobytes(), rows, [bk.m.token_counts(b).tobytes() for b in range(B)]))
        bk.close()
    assert out[0] == out[1]
