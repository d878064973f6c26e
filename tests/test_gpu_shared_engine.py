"""Shared-prefix attention in the engine (gpt2_decode_set_shared_attention):
forks of one prompt decode with their shared tiles streamed once per unit.

tests/test_gpu_fork.py's SMALL config, helpers and bars: logits within
LOGIT_TOL = 2e-4 of one oracle per sequence fed its full history, greedy ids
equal where the oracle's margin exceeds TIE_MARGIN = 1e-3.  Page sizes 16 and
8, graph on, the plan's thresholds set to (1 tile, 2 members, 2 sequences
covered) so that the small config's prefixes form units whatever the measured
defaults are.  The engine's
plan is compared with the numpy restatement (tests/shared_ref64.py) over the
manager's own page lists.
"""
import numpy as np
import pytest

import shared_ref64 as sr
from test_gpu_fork import LOGIT_TOL, SMALL, Forks

pytestmark = pytest.mark.gpu


def _manager(hip, B, P, pages=None):
    per = SMALL["maxT"] // P
    return hip.BlockManager(SMALL["C"], max_prompts=B, max_blocks=pages or B * per, block_size=P,
                            max_blocks_per_prompt=per)


def _numpy_plan(s, bm):
    per = SMALL["maxT"] // s.P
    bt = np.full((s.B, per), -1, np.int32)
    for b in range(s.B):
        pg = bm.pages(b)
        bt[b, :len(pg)] = pg
    pos = np.array(s.model.positions())
    units, skip = sr.plan(bt, pos, s.P, 1, 2)
    unit_of = np.full(s.B, -1, np.int32)
    for u, (m, _) in enumerate(units):
        unit_of[m] = u
    return len(units), unit_of, 64 * skip


def _check_plan(s, bm):
    n, unit_of, tok = s.model.shared_plan()
    wn, wu, wt = _numpy_plan(s, bm)
    assert n == wn and np.array_equal(unit_of, wu) and np.array_equal(tok, wt), (n, unit_of, tok, wn, wu, wt)
    return n, unit_of, tok


def _scenario(hip, P, seed, B=9, pages=None):
    """slot 0: a 150-token prompt; slots 1-5 fork all of it, slot 6 its first 70 tokens, slot 7 its first 40
    (no tile); slot 8 an unrelated prompt"""
    bm = _manager(hip, B, P, pages)
    s = Forks(hip, B=B, P=P, seed=seed, bm=bm)
    s.model.set_graph(True)
    s.model.set_shared_attention(True, min_tiles=1, min_members=2, min_covered=2)
    assert s.model.shared_attention() and s.model.shared_thresholds() == (1, 2, 2)
    s.run({0: s.admit(0, 150)})
    assert s.model.shared_plan()[0] == 0  # nothing shared yet
    for b in range(1, 6):
        s.fork(0, b)
    s.fork(0, 6, 70)
    s.fork(0, 7, 40)
    s.run({8: s.admit(8, 30)})
    return s, bm


@pytest.mark.parametrize("P", [16, 8])
def test_forks_of_different_lengths(hip, P):
    s, bm = _scenario(hip, P, seed=31)
    n, unit_of, tok = _check_plan(s, bm)
    assert n == 1 and unit_of.tolist() == [0] * 6 + [-1] * 3 and tok.tolist() == [128] * 6 + [0] * 3
    # different tokens per slot until a member's suffix (from token 128 on) is two tiles long: past 192,
    # across the page edges on the way
    for step in range(46):
        s.decode([s.cur[0]] + s.tokens(s.B - 1))
        if step == 0:
            assert s.model.shared_plan()[0] == 1
    assert s.model.positions()[0] == 196
    _check_plan(s, bm)  # appends never change the plan
    print(f"SHAREDENG forks P={P}: worst |logit diff| {s.worst:.2e}")
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()
    bm.close()


@pytest.mark.parametrize("P", [16, 8])
def test_plan_change_under_a_graph(hip, P):
    s, bm = _scenario(hip, P, seed=32)
    for _ in range(3):
        s.decode([s.cur[0]] + s.tokens(s.B - 1))
    assert _check_plan(s, bm)[1].tolist() == [0] * 6 + [-1] * 3
    # a member leaves mid-run: the unit shrinks, the graph stays
    s.drop(3)
    n, unit_of, _ = _check_plan(s, bm)
    assert n == 1 and unit_of.tolist() == [0, 0, 0, -1, 0, 0, -1, -1, -1]
    # a new prompt in its slot, forked again into a slot that leaves for it: a second unit
    s.run({3: s.admit(3, 100)})
    s.drop(7)
    s.fork(3, 7)
    n, unit_of, tok = _check_plan(s, bm)
    assert n == 2 and unit_of.tolist() == [0, 0, 0, 1, 0, 0, -1, 1, -1] and tok[3] == tok[7] == 64
    for _ in range(4):
        s.decode([s.cur[0]] + s.tokens(s.B - 1))
    _check_plan(s, bm)
    print(f"SHAREDENG plan change P={P}: worst |logit diff| {s.worst:.2e}")
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()
    bm.close()


@pytest.mark.parametrize("P", [16, 8])
def test_rewind_below_the_shared_length(hip, P):
    s, bm = _scenario(hip, P, seed=33)
    s.decode([s.cur[0]] + s.tokens(s.B - 1))
    pos = list(s.model.positions())

    def rewind(b, n):
        pos[b] = n
        s.model.set_positions(pos)
        s.reqs[b].close()
        s.hist[b] = s.hist[0][:n]
        s.reqs[b] = s._request()
        s.reqs[b].feed(s.hist[b])

    rewind(2, 100)  # one whole tile left under it: it leaves the unit of 2 tiles and pairs with slot 6 over 1 tile
    rewind(4, 30)   # below a tile: out
    n, unit_of, tok = _check_plan(s, bm)
    assert n == 2 and unit_of.tolist() == [0, 0, 1, 0, -1, 0, 1, -1, -1]
    assert tok.tolist() == [128, 128, 64, 128, 0, 128, 64, 0, 0]
    free = bm.free_pages()
    s.decode([s.cur[0]] + s.tokens(s.B - 1))   # slots 2 and 4 append into private copies of shared pages
    assert bm.free_pages() <= free - 2
    _check_plan(s, bm)
    for _ in range(3):
        s.decode([s.cur[0]] + s.tokens(s.B - 1))
    print(f"SHAREDENG rewind P={P}: worst |logit diff| {s.worst:.2e}")
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()
    bm.close()


def test_eviction_of_a_holder(hip):
    """a pool with no page to spare: an append pages out the LRU holder of the prefix, the plan follows
    and the two holders left decode on as a unit"""
    P, B = 16, 4
    bm = _manager(hip, B, P, pages=14)
    s = Forks(hip, B=B, P=P, seed=34, bm=bm)
    s.model.set_graph(True)
    s.model.set_shared_attention(True, min_tiles=1, min_members=2, min_covered=2)
    s.run({0: s.admit(0, 84)})       # 5 full pages + a tail
    s.fork(0, 1)                     # 5 shared + its own tail
    s.fork(0, 2)
    assert _check_plan(s, bm)[1].tolist() == [0, 0, 0, -1]
    s.run({3: s.admit(3, 90)})       # 6 pages: all 14 in use
    assert bm.free_pages() == 0 and not s.model.evicted().any()
    # position 96 of slot 3 needs a seventh page: the source is paged out for its private tail page (the
    # LRU page with one holder, as in tests/test_gpu_fork.py), the shared pages stay with the forks
    x = 0
    s.reqs[x].close()
    s.reqs[x], s.hist[x] = None, []
    s.run({3: s.tokens(7)})
    assert list(s.model.evicted()) == [True, False, False, False]
    n, unit_of, tok = _check_plan(s, bm)
    assert n == 1 and unit_of[x] == -1 and unit_of[3] == -1 and (unit_of >= 0).sum() == 2
    s.drop(3)                        # room again: both free slots take a short prompt, then everybody decodes
    s.run({3: s.admit(3, 10), x: s.admit(x, 12)})
    for _ in range(3):
        s.decode(s.tokens(B))
    assert _check_plan(s, bm)[0] == 1
    assert s.worst <= LOGIT_TOL, s.worst
    s.close()
    bm.close()


def test_bit_equality_without_forks_and_after_off(hip):
    """on with nothing shared, and off again after use: the logits of an engine that never enabled it"""
    rng = np.random.default_rng(35)
    prompts = [[int(t) for t in rng.integers(0, SMALL["V"], 70 + 3 * b)] for b in range(4)] + [[]]
    extra = rng.integers(0, SMALL["V"], 5).astype(np.int32)
    steps = rng.integers(0, SMALL["V"], (3, 5)).astype(np.int32)

    def run(mode):
        s = Forks(hip, B=5, P=16, seed=35, oracle=False)
        s.model.set_graph(True)
        if mode == "on":
            s.model.set_shared_attention(True, min_tiles=1, min_members=2, min_covered=2)
        s.model.prefill_ragged(prompts)
        if mode == "used_then_off":
            s.model.set_shared_attention(True, min_tiles=1, min_members=2, min_covered=2)
            s.model.fork(0, 4)
            s.model.step(extra)
            assert s.model.shared_plan()[0] == 1
            s.model.release(4)
            s.model.set_positions([len(p) for p in prompts])  # the step's appends are overwritten below
            s.model.set_shared_attention(False)
            assert s.model.shared_plan()[0] == 0
        out = []
        for t in steps:
            s.model.step(t)
            out.append(s.model.logits().copy())
        if mode == "on":
            assert s.model.shared_plan()[0] == 0
        s.close()
        return np.stack(out)

    base = run("never")
    assert np.abs(base).max() > 0 and np.isfinite(base).all()
    assert np.array_equal(run("on").view(np.uint32), base.view(np.uint32))
    assert np.array_equal(run("used_then_off").view(np.uint32), base.view(np.uint32))


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_refused_on_other_pools(hip, kv):
    dt = dict(bf16=hip.HPA_BF16, fp8=hip.HPA_FP8)[kv]
    s = Forks(hip, B=2, P=16, seed=36, kv_dtype=dt, oracle=False)
    with pytest.raises(RuntimeError):
        s.model.set_shared_attention(True)
    assert not s.model.shared_attention() and s.model.shared_plan()[0] == 0
    s.model.set_shared_attention(False)  # off is always accepted
    s.model.prefill_ragged([s.tokens(20), s.tokens(5)])
    s.close()


def test_default_thresholds_leave_a_small_batch_alone(hip):
    """the measured defaults (15 tiles, 2 members, units covering 64 sequences): three forks of a short
    prompt form no unit, and the step is the plain step bit for bit"""
    def run(on):
        s = Forks(hip, B=3, P=16, seed=37, oracle=False)
        s.model.set_graph(True)
        if on:
            s.model.set_shared_attention(True)
            assert s.model.shared_thresholds() == (15, 2, 64)
        s.model.prefill_ragged([s.tokens(100), [], []])
        s.model.fork(0, 1)
        s.model.fork(0, 2)
        out = []
        for _ in range(2):
            s.model.step(np.array(s.tokens(3), np.int32))
            out.append(s.model.logits().copy())
        if on:
            assert s.model.shared_plan()[0] == 0
        s.close()
        return np.stack(out)

    assert np.array_equal(run(True).view(np.uint32), run(False).view(np.uint32))
