"""tests/engine_model.py on the CPU: the float64 decoder against itself and the
pinned fp32 oracle, what each class of engine fault moves, the conditions
every trace of tests/test_gpu_engine_traces.py meets, and the checker against
injected faults.

Figures of this file (x86-64, numpy float64; `pytest -s` prints them):

Reference distance -- worst |fp32 oracle PagedDecoder - Decoder64| over every
row of the final histories of the fp32 profiles' traces: see
profiles/EXPERIMENTS.md "Engine call traces"; asserted <= bar / 16 = 1.25e-5.

Sensitivity -- the movement of the last row's logits (max over the vocabulary)
when only the reference's input is corrupted, asserted >= 10 x bar unless the
(class, length) pair is listed in BIT_LEVEL_ONLY, the pairs that only the
bit-level checks 3-5 (untouched rows, K/V prefixes, pages) see at that bar.
"""
import copy

import numpy as np
import pytest

import engine_model as em
import oracle_ctypes as oc
import pagedattn
import synth
from engine_model import BF16_LOGIT_TOL, LOGIT_TOL, SMALL

CASES = [(name, seed) for name, p in em.PROFILES.items() for seed in p["seeds"]]
IDS = [f"{n}-{s}" for n, s in CASES]


def c_plan(bt, pos, P):
    """gpt2_attn_shared_plan (pure, host only) in plan_units' shape, thresholds (1 tile, 2 members)"""
    n, members, tiles, skip = pagedattn.attn_shared_plan(bt, pos, P, 1, 2)
    unit_of = np.full(len(pos), -1, np.int32)
    for u in range(n):
        unit_of[[b for b in members[u] if b >= 0]] = u
    return n, unit_of, 64 * skip


def run_model(profile, seed, n_ops=None, visit=None):
    """the trace with the model's own observations (and the stand-in eviction mask of the evict profile);
    visit(i, op, exp, prev, obs, model) runs before the clean check.  Returns (model, log)"""
    trace = em.make_trace(profile, seed, n_ops)
    m = trace.model
    prev, log = m.observe(plan_fn=c_plan), []
    for i, op in enumerate(trace):
        mask = m.standin_evictions(op) if m.evicting else None
        before = dict(pos=[m.pos(b) for b in range(m.B)], pages=[list(pl) for pl in m.pages], graph=m.graph,
                      units=c_plan(m.block_table(), [m.pos(b) for b in range(m.B)], m.P)[0])
        exp = m.apply(op, mask)
        obs = m.observe(exp, plan_fn=c_plan)
        if visit:
            visit(i, op, exp, prev, obs, m)
        em.check_op(m, exp, prev, obs, i)
        before["units_after"] = c_plan(m.block_table(), obs.pos, m.P)[0]
        log.append((op, exp, before))
        prev = obs
    return m, log


@pytest.fixture(scope="module")
def runs():
    """every (profile, seed) of the GPU file, run once on the model alone"""
    return {c: run_model(*c) for c in CASES}


# ---------------------------------------------------------------- the decoder
@pytest.mark.parametrize("kv_bf16", [False, True], ids=["f32", "kv_bf16"])
def test_decoder_self_consistency(kv_bf16):
    """token by token, in chunks, forked and rewound: the rows of one from-scratch pass, to 1e-10"""
    ref = em.make_ref(SMALL, synth.params(SMALL, seed=1), kv_bf16=kv_bf16)
    rng = np.random.default_rng(3)
    toks = [int(t) for t in rng.integers(0, SMALL["V"], 90)]
    want = em.forward64(ref, toks)
    one = em.Decoder64(ref)
    got = np.stack([one.feed([t])[0] for t in toks])
    assert np.abs(got - want).max() <= 1e-10
    chunks = em.Decoder64(ref)
    got = np.concatenate([chunks.feed(toks[a:b]) for a, b in [(0, 1), (1, 17), (17, 18), (18, 70), (70, 90)]])
    assert np.abs(got - want).max() <= 1e-10
    f = chunks.fork(37)          # a fork continues with the source's tokens ...
    assert np.abs(f.feed(toks[37:60]) - want[37:60]).max() <= 1e-10
    other = toks[:37] + [int(t) for t in rng.integers(0, SMALL["V"], 20)]
    g = chunks.fork(37)          # ... or with its own, and the source does not notice
    assert np.abs(g.feed(other[37:]) - em.forward64(ref, other)[37:]).max() <= 1e-10
    chunks.rewind(50)
    chunks.feed([1, 2, 3])       # rows the rewind below discards
    chunks.rewind(50)
    assert np.abs(chunks.feed(toks[50:]) - want[50:]).max() <= 1e-10
    for l in range(SMALL["L"]):
        assert np.array_equal(chunks.K[l, :90], one.K[l, :90]) or np.abs(chunks.K[l, :90] - one.K[l, :90]).max() < 1e-12


def test_reference_distance(runs):
    """the fp32 oracle against Decoder64 on the histories the fp32 profiles' traces end with: at most bar / 16,
    so the bar is loose for the reference alone and means what it meant against the oracle"""
    worst = {}
    for (profile, seed), (m, _) in runs.items():
        if m.kv_bf16:
            continue
        hists = sorted((h for h in m.hist if h), key=len, reverse=True)
        hists = hists[:1] if profile == "chain6" else hists  # C = 768: the longest one (the oracle's cost)
        c = oc.cfg(m.maxT, m.V, m.cfg["L"], m.cfg["NH"], m.cfg["C"])
        for h in hists:
            o = oc.PagedDecoder(m.params, c, 1, m.P, m.maxT, page_seed=seed)
            got = np.stack([o.step(np.array([t], np.int32))[1][0] for t in h])
            o.close()
            d = float(np.abs(got - em.forward64(m.ref, h)).max())
            worst[profile] = max(worst.get(profile, 0.0), d)
    for profile, d in worst.items():
        print(f"REFDIST {profile}: worst |fp32 oracle - float64| {d:.2e} (bar {LOGIT_TOL:.0e}, bar / 16 {LOGIT_TOL / 16:.2e})")
    assert set(worst) == {"f32-all", "f32-shared-graph", "evict", "chain6"}
    assert max(worst.values()) <= LOGIT_TOL / 16, worst


# ---------------------------------------------------------------- sensitivity
CLASSES = ("wrong token", "page of another slot", "context short by one key", "context long by one stale key",
           "fork prefix n + 1", "fork prefix n - 1", "rejected draft row left")
LENGTHS = (20, 100, 200)
# (pool, class, length) whose movement stays under 10 x bar: seen by the bit-level checks 3-5 only
BIT_LEVEL_ONLY = {
    ("bf16", "wrong token", 100), ("bf16", "wrong token", 200),
    ("bf16", "page of another slot", 200),
    ("bf16", "context short by one key", 20), ("bf16", "context short by one key", 100),
    ("bf16", "context short by one key", 200),
    ("bf16", "context long by one stale key", 100), ("bf16", "context long by one stale key", 200),
}


def _movements(ref, P=16, seed=5):
    rng = np.random.default_rng(seed)
    out = {}
    for n in LENGTHS:
        h = [int(t) for t in rng.integers(0, ref.cfg["V"], n)]
        other = [int(t) for t in rng.integers(0, ref.cfg["V"], n)]
        d = em.Decoder64(ref)
        d.feed(h[:-1])
        o = em.Decoder64(ref)
        o.feed(other)
        right = d.fork(n - 1).feed(h[-1:])[0]
        last = lambda toks: em.forward64(ref, toks)[-1]  # noqa: E731
        k = n // 2
        wrong = list(h)
        wrong[k] = (h[k] + 1) % ref.cfg["V"]
        swapped = d.fork(n - 1)
        pg = min(1, (n - 2) // P) * P  # page 1 where the history has one, else page 0
        hi = min(pg + P, n - 1)
        for a in ("K", "V"):
            getattr(swapped, a)[:, pg:hi] = getattr(o, a)[:, pg:hi]
        stale = d.fork(n - 1)
        for a in ("K", "V"):  # the slot past the new row holds another sequence's row
            getattr(stale, a)[:, n] = getattr(o, a)[:, n - 1]
        rows = {
            "wrong token": last(wrong),
            "page of another slot": swapped.feed(h[-1:])[0],
            "context short by one key": d.fork(n - 1).feed(h[-1:], ctx_shift=-1)[0],
            "context long by one stale key": stale.feed(h[-1:], ctx_shift=1)[0],
            "fork prefix n + 1": last(h[:k] + [other[k]] + h[k:]),
            "fork prefix n - 1": last(h[:k] + h[k + 1:]),
            "rejected draft row left": last(h[:n - 3] + [other[0]] + h[n - 3:]),
        }
        for c in CLASSES:
            out[c, n] = float(np.abs(rows[c] - right).max())
    return out


@pytest.mark.parametrize("pool,bar", [("f32", LOGIT_TOL), ("bf16", BF16_LOGIT_TOL)])
def test_sensitivity(pool, bar):
    """one corruption of each class in the reference's input, histories of 20, 100 and 200 tokens: the
    movement of the last row is at least 10 x bar, except where BIT_LEVEL_ONLY names the pair"""
    ref = em.make_ref(SMALL, synth.params(SMALL, seed=1), kv_bf16=pool == "bf16")
    mv = _movements(ref)
    print(f"SENSITIVITY {pool} pool, bar {bar:.0e} (10 x bar = {10 * bar:.0e}); movement of the last row at {LENGTHS}")
    for c in CLASSES:
        marks = ["" if mv[c, n] >= 10 * bar else " (bits only)" for n in LENGTHS]
        print(f"  {c:32s}" + "".join(f" {mv[c, n]:9.2e}{k}" for n, k in zip(LENGTHS, marks)))
    below = {(pool, c, n) for c in CLASSES for n in LENGTHS if mv[c, n] < 10 * bar}
    assert below == {x for x in BIT_LEVEL_ONLY if x[0] == pool}, sorted(below ^ {x for x in BIT_LEVEL_ONLY if x[0] == pool})


# ---------------------------------------------------------------- the traces
def _passes(op):
    return op["kind"] in ("admit", "ragged", "step_host", "step_dev", "verify", "verify_tree")


@pytest.mark.parametrize("profile,seed", CASES, ids=IDS)
def test_trace_conditions(runs, profile, seed):
    m, log = runs[profile, seed]
    p, P = em.PROFILES[profile], m.P
    kinds = [op["kind"] for op, _, _ in log]
    assert len(log) == p["n_ops"]
    assert set(kinds) == set(p["kinds"]), set(p["kinds"]) ^ set(kinds)
    assert m.exempt <= 0.05 * m.picks, (m.exempt, m.picks)
    print(f"TRACE {profile} seed {seed}: exempt near-tie rows {m.exempt} / {m.picks} picks")
    # forks of every kind
    forks = [(exp.fork[2], before["pos"][exp.fork[0]]) for op, exp, before in log if exp.fork]
    assert any(n % P == 0 for n, _ in forks) and any(n % P for n, _ in forks) and any(n < s for n, s in forks), forks
    if "step_dev" in p["kinds"]:
        assert kinds.count("step_dev") >= 2
    if "verify" in p["kinds"]:
        acc = [(v[0], len(d)) for op, exp, _ in log if op["kind"] == "verify"
               for v, d in zip(exp.verify, op["drafts"]) if v is not None]
        assert any(a == 0 and n > 0 for a, n in acc) and any(0 < a < n for a, n in acc) and \
            any(a == n > 0 for a, n in acc), acc
        assert {-1, 0} <= {(-1 if d is None else len(d)) for op, _, _ in log if op["kind"] == "verify"
                           for d in op["drafts"]}
        assert any(a == "verify" and b == "step_dev" for a, b in zip(kinds, kinds[1:]))
        # a fork lands in a slot that was released after a verify pass left rejected rows in its pages
        state, hit = {}, False
        for op, exp, _ in log:
            if op["kind"] in ("verify", "verify_tree"):
                args = op["drafts"] if op["kind"] == "verify" else [t and t[0] for t in op["trees"]]
                for b, v in enumerate(exp.verify):
                    if v is not None and v[0] < len(args[b]):
                        state[b] = "rejected"
            elif op["kind"] == "release":
                state[op["slot"]] = "released" if state.get(op["slot"]) == "rejected" else None
            elif op["kind"] == "fork":
                hit |= state.get(op["dst"]) == "released"
                state[op["dst"]] = None
            elif _passes(op):
                for b in exp.touched:
                    state[b] = None
            elif op["kind"] == "reset":
                state = {}
        assert hit
    if "verify_tree" in p["kinds"]:
        walks = [v[0] for op, exp, _ in log if op["kind"] == "verify_tree" for v in exp.verify if v is not None]
        assert any(a > 0 for a in walks), walks
    if "rewind" in p["kinds"]:
        into_shared = boundary = below_shared = False
        pending = {}  # slot -> rewound into a shared page, no append yet
        for op, exp, before in log:
            if op["kind"] == "rewind":
                for b, n in enumerate(op["pos"]):
                    if n == before["pos"][b]:
                        continue
                    pl = before["pages"][b]
                    held = lambda pg: sum(pg in q for q in before["pages"])  # noqa: E731
                    shared_len = sum(1 for pg in pl if held(pg) > 1) * P
                    boundary |= n % P == 0
                    below_shared |= n < shared_len
                    if n % P and held(pl[n // P]) > 1:
                        pending[b] = n // P
            elif _passes(op):
                for b in exp.touched:
                    if b in pending:
                        into_shared |= (b, pending.pop(b)) in exp.cow
            elif op["kind"] in ("release", "reset", "fork"):
                pending = {}
        assert into_shared and boundary and below_shared, (into_shared, boundary, below_shared)
    if "set_graph" in p["kinds"]:
        assert any(_passes(op) and before["graph"] for op, _, before in log)
        # right after each toggle a pass runs: the very next op, before anything else changes the engine
        for i, k in enumerate(kinds[:-1]):
            if k.startswith("set_"):
                assert _passes(log[i + 1][0]), (i, k, kinds[i + 1])
    if p["shared"]:
        assert any(before["units"] >= 1 and _passes(op) for op, _, before in log)
        assert any(before["units"] > before["units_after"] and op["kind"] in ("rewind", "release")
                   for op, _, before in log)


def test_prefix_of_a_trace_is_a_trace():
    """op i does not depend on n_ops: a failure at op i reproduces with n_ops = i + 1"""
    _, full = run_model("f32-all", 1, 40)
    _, head = run_model("f32-all", 1, 23)
    assert [op for op, _, _ in head] == [op for op, _, _ in full[:23]]


# ---------------------------------------------------------------- the checker
def _flip(a, index):
    a.view(np.uint32)[index] ^= 1


def _faults(op, exp, prev, obs, m):
    """(name of the check that must fire, corrupted copy of obs) for every fault this op lends itself to"""
    out = []
    B = m.B

    def corrupt(check, fn):
        o = copy.deepcopy(obs)
        if fn(o) is not False:
            out.append((check, fn.__name__, o))

    touched = sorted(exp.touched)
    others = [b for b in range(B) if b not in exp.touched]
    if touched:
        b = touched[0]

        def moved(o):            # a logits row moved by 2 x bar (every column: the argmax stays)
            o.logits[b] += np.float32(2 * m.bar)
        corrupt("logits", moved)

        def own(o):              # a next id that is not the argmax of the engine's own row
            o.next_ids[b] = (o.next_ids[b] + 1) % m.V
        corrupt("next-id-own-argmax", own)

        def f64(o):              # another column on top, consistently: not the float64 argmax
            if exp.touched[b]["tie"]:
                return False
            j = (int(o.next_ids[b]) + 7) % m.V
            o.logits[b, j] = o.logits[b].max() + 1.0
            o.next_ids[b] = j
            if isinstance(o.result, np.ndarray):
                o.result[b] = j
            else:
                o.result[1][b][-1] = j
        corrupt("next-id-float64", f64)

        def value(o):            # a written K row off by one part in 1000
            o.kv[0][b][0][o.pos[b] - 1] *= np.float32(1.001)
        corrupt("kv-written", value)

        def pos(o):
            o.pos[b] += 1
        corrupt("position", pos)
        sib = [x for x in others if prev.pos[x] > 0 and obs.pos[x] == prev.pos[x]]
        if sib:
            def prefix(o):       # one bit of a sibling's prefix
                _flip(o.kv[m.cfg["L"] - 1][sib[0]][1], (prev.pos[sib[0]] // 2, 5))
            corrupt("kv-prefix", prefix)
        if obs.pages is not None:
            def two(o):          # the page just written has a second holder
                x = (b + 1) % B
                i = (o.pos[b] - 1) // m.P
                pg = o.pages[b][i]
                while len(o.pages[x]) <= i:
                    o.pages[x].append(-len(o.pages[x]) - 1000 * (x + 1))
                    o.refs[o.pages[x][-1]] = 1
                o.pages[x][i] = pg
                o.refs[pg] = 2
            corrupt("written-page-private", two)
    fed_others = [x for x in others if exp.fed_before[x]]
    if fed_others:
        def row(o):
            _flip(o.logits[fed_others[0]], 3)
        corrupt("untouched", row)

        def nid(o):
            if exp.full_fork and fed_others[0] == exp.fork[1]:
                return False
            o.next_ids[fed_others[0]] += 1
        corrupt("untouched", nid)

    def free(o):
        o.free_pages -= 1
    corrupt("free-pages", free)
    if touched and isinstance(obs.result, np.ndarray):
        def returned(o):         # the call reports another id than the device holds
            o.result[touched[0]] += 1
        corrupt("next-id-own-argmax", returned)
    if exp.verify is not None:
        def acc(o):
            b = [i for i, v in enumerate(exp.verify) if v is not None][0]
            o.result[0][b] += 1
        corrupt("verify-walk", acc)
        took = [i for i, v in enumerate(exp.verify) if v is not None and v[0] >= 1]
        if took:
            def tokens(o):       # the right count, another accepted token
                o.result[1][took[0]][0] += 1
            corrupt("verify-walk", tokens)

        def last(o):             # the pass's own token is not the id the device holds
            b = [i for i, v in enumerate(exp.verify) if v is not None][0]
            o.result[1][b][-1] += 1
        corrupt("verify-walk", last)
        if exp.kind == "verify_tree":
            def nodes(o):        # the right tokens through another node
                b = [i for i, v in enumerate(exp.verify) if v is not None][0]
                o.result[2][b] = [x + 1 for x in o.result[2][b]] or [1]
            corrupt("verify-walk", nodes)
        idle = [i for i, v in enumerate(exp.verify) if v is None]
        if idle:
            def woke(o):         # a count for a slot the pass was told to leave alone
                o.result[0][idle[0]] = 0
            corrupt("verify-walk", woke)
    if obs.pages is not None:
        quiet = [x for x in others if obs.pages[x]]
        if quiet:
            def refs(o):         # a holder count that is not the number of lists the page is in
                o.refs[o.pages[quiet[0]][0]] += 1
            corrupt("page-sharing", refs)
        apart = [(x, y) for x in quiet for y in quiet if x < y and obs.pages[x][0] != obs.pages[y][0]]
        if apart:
            def joined(o):       # two slots share a page the model keeps apart
                x, y = apart[0]
                old, pg = o.pages[y][0], o.pages[x][0]
                o.pages[y][0] = pg
                o.refs[pg] += 1
                if not any(old in pl for pl in o.pages):
                    del o.refs[old]
                else:
                    o.refs[old] -= 1
            corrupt("page-sharing", joined)
    if exp.fork:
        def fk(o):
            _flip(o.kv[0][exp.fork[1]][0], (exp.fork[2] - 1, 0))
        corrupt("fork-copy", fk)
    if obs.pages is not None and exp.kind == "release":
        def pattern(o):          # a released slot still lists a page
            o.pages[op["slot"]] = [10 ** 6]
            o.refs[10 ** 6] = 1
        corrupt("page-sharing", pattern)
    if obs.plan is not None and obs.plan[0] >= 1:
        n_units, unit_of, tok = obs.plan
        outsiders = [x for x in range(B) if unit_of[x] < 0]
        members = [x for x in range(B) if unit_of[x] == 0]

        def alone(o):            # a unit of one member
            for x in members[1:]:
                o.plan[1][x], o.plan[2][x] = -1, 0
        corrupt("shared-plan", alone)

        def ragged_tile(o):      # not whole tiles
            for x in members:
                o.plan[2][x] += 1
        corrupt("shared-plan", ragged_tile)

        def too_long(o):         # more shared tokens than a member has cached
            for x in members:
                o.plan[2][x] = 64 * (min(obs.pos[y] for y in members) // 64 + 1)
        corrupt("shared-plan", too_long)
        if outsiders:
            def no_such_unit(o):
                o.plan[1][outsiders[0]] = n_units
            corrupt("shared-plan", no_such_unit)

            def stray_tokens(o):  # shared tokens for a slot in no unit
                o.plan[2][outsiders[0]] = 64
            corrupt("shared-plan", stray_tokens)

        def uneven(o):           # one member streams a tile more than its unit
            o.plan[2][members[1]] += 64
        corrupt("shared-plan", uneven)
        long_enough = [x for x in outsiders if obs.pos[x] >= tok[members[0]]]
        if long_enough:
            def unit(o):         # a unit with a member that has the tokens, in other pages
                o.plan[1][long_enough[0]] = 0
                o.plan[2][long_enough[0]] = o.plan[2][members[0]]
            corrupt("shared-plan", unit)
    return out


def test_checker_faults():
    """check_op fed the model's own values passes (every run above); one corrupted observation per check
    raises and names that check"""
    fired = {}

    def visit(i, op, exp, prev, obs, m):
        for check, variant, bad in _faults(op, exp, prev, obs, m):
            if fired.get((check, variant), 0) >= 2:
                continue
            with pytest.raises(em.CheckFailed) as e:
                em.check_op(m, exp, prev, bad, i)
            assert e.value.check == check, (check, variant, str(e.value))
            assert f"profile {m.profile}, seed {m.seed}, op {i}" in str(e.value)
            fired[check, variant] = fired.get((check, variant), 0) + 1

    run_model("f32-shared-graph", 1, visit=visit)
    # a scripted state for the one fault the trace need not lend itself to: a slot with the unit's tokens in
    # pages of its own (two 70-token prompts, a fork of the first)
    m = em.EngineModel("f32-shared-graph", 1)
    prev = m.observe(plan_fn=c_plan)
    for i, op in enumerate([dict(kind="admit", seqs=[list(range(70)), [], list(range(100, 170)), [], [], []]),
                            dict(kind="fork", src=0, dst=1, n=-1)]):
        exp = m.apply(op)
        obs = m.observe(exp, plan_fn=c_plan)
        visit(i, op, exp, prev, obs, m)
        em.check_op(m, exp, prev, obs, i)
        prev = obs
    assert obs.plan[0] == 1
    want = {("logits", "moved"), ("next-id-own-argmax", "own"), ("next-id-own-argmax", "returned"),
            ("next-id-float64", "f64"), ("kv-written", "value"), ("position", "pos"), ("kv-prefix", "prefix"),
            ("written-page-private", "two"), ("untouched", "row"), ("untouched", "nid"), ("free-pages", "free"),
            ("verify-walk", "acc"), ("verify-walk", "woke"), ("verify-walk", "tokens"), ("verify-walk", "last"),
            ("verify-walk", "nodes"), ("shared-plan", "stray_tokens"), ("shared-plan", "uneven"), ("fork-copy", "fk"), ("page-sharing", "pattern"),
            ("page-sharing", "refs"), ("page-sharing", "joined"), ("shared-plan", "alone"),
            ("shared-plan", "ragged_tile"), ("shared-plan", "too_long"), ("shared-plan", "no_such_unit"),
            ("shared-plan", "unit")}
    assert set(fired) == want, want ^ set(fired)


def test_checker_refuses_an_eviction_with_room():
    """the evict profile: a slot reported evicted by an op that had the pages it needed"""
    m = em.EngineModel("evict", 1)
    prev = m.observe()
    op = dict(kind="admit", seqs=[[1, 2, 3], [4, 5], [], []])
    exp = m.apply(op)
    obs = m.observe(exp)
    em.check_op(m, exp, prev, obs, 0)
    prev, op = obs, dict(kind="step_host", tokens=[7, 8, 9, 10])
    exp = m.apply(op, [True, False, False, False])
    with pytest.raises(em.CheckFailed) as e:
        em.check_op(m, exp, prev, m.observe(exp), 1)
    assert e.value.check == "eviction"


def test_checker_in_the_evict_profile():
    """evictions are not predicted: the free count is held to the engine's own lists, and a holder of nothing
    but shared pages is never the one paged out"""
    m = em.EngineModel("evict", 1)
    prev = m.observe()
    for i, op in enumerate([dict(kind="admit", seqs=[list(range(16)), [], [], list(range(150))]),
                            dict(kind="fork", src=0, dst=1, n=16)]):
        exp = m.apply(op)
        obs = m.observe(exp)
        em.check_op(m, exp, prev, obs, i)
        prev = obs
    assert m.free_pages() == 1 and m.pages[1] == m.pages[0]
    bad = copy.deepcopy(prev)
    bad.free_pages += 1
    with pytest.raises(em.CheckFailed) as e:
        em.check_op(m, exp, prev, bad, 1)  # the fork's own check again, on a free count its lists do not give
    assert e.value.check == "free-pages"
    # a step pages slot 1 out (every slot of a step gains a page of its own, so that is allowed) -- and the page
    # it shared must stay where slot 0 had it
    m2 = copy.deepcopy(m)
    exp = m2.apply(dict(kind="step_host", tokens=[1, 2, 3, 4]), [False, True, False, False])
    obs = m2.observe(exp)
    em.check_op(m2, exp, prev, obs, 2)
    bad = copy.deepcopy(obs)
    old = bad.pages[0][0]
    bad.pages[0][0] = 10 ** 6
    bad.refs[10 ** 6] = bad.refs.pop(old)
    with pytest.raises(em.CheckFailed) as e:
        em.check_op(m2, exp, prev, bad, 2)
    assert e.value.check == "eviction" and "did not stay" in str(e.value)
    exp = m.apply(dict(kind="admit", seqs=[[], [], list(range(40)), []]), [False, True, False, False])
    with pytest.raises(em.CheckFailed) as e:
        em.check_op(m, exp, prev, m.observe(exp), 2)
    assert e.value.check == "eviction" and e.value.slot == 1
