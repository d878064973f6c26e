"""Engine-level sampled tree speculation: gpt2_decode_verify_tree_sampled on the
model, batch and truth of tests/test_gpu_speculate.py (SMALL, B = 4, page 16).

Bars.  eps = 2 * LOGIT_TOL / T is test_gpu_speculate_sampled's relative bound on
one mass under temperature T.  A child examined after rejected siblings of
total mass s is judged against the conditional mass q = p / (1 - s); the
first-order propagation of eps through that quotient is eps * q * (1 + s / (1 -
s)), and the bound used is twice that (the higher-order terms), plus that
module's 2^-40 quantum where the mass itself lies below it.  Decisions are
compared exactly: _plan first asserts, from the oracle alone (teacher-forced
logits of every internal node, float64 masses, the Python coin stream, the
walk), that every examined coin clears its bound.  TREE_SEED and TREE_TEMPS were
found by a search on the CPU over seeds at the LOW_TEMPS scale; the plan must
contain a sampled sequence that accepts a non-first sibling after rejecting an
earlier one, a sequence that rejects every child of a node with two children,
and a sequence that ends on a leaf -- asserted from the plan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc
import sample_ref64 as sr
import synth
import tree_spec_ref64 as ts
from test_gpu_kv_append import KV_RTOL
from test_gpu_score import LOGIT_TOL, SMALL, TIE_MARGIN, V
from test_gpu_speculate import B, MR, P, PRE, _forced, _model, _pending, _teacher_forced, _Truth, params, truth  # noqa: F401
from test_gpu_speculate_sampled import LOW_TEMPS, TEMPS, _coins, _mass64, _sampled
from test_gpu_speculate_tree import _nonfirst, _prepared

pytestmark = pytest.mark.gpu
_I = ctypes.POINTER(ctypes.c_int)
_F = ctypes.POINTER(ctypes.c_float)
QUANTUM = 2.0 ** -40


def _kv_worst(m, orc_kv, b, n):
    worst = 0.0
    for l in range(SMALL["L"]):
        k, v = m.read_kv(l, b, n)
        ko, vo = orc_kv(l, n)
        for got, ref in ((k, ko), (v, vo)):
            r = np.abs(got.astype(np.float64) - ref).max(-1) / np.abs(ref).max(-1)
            worst = max(worst, float(r.max()))
    return worst


# ---------------------------------------------------------------- 1. T = 0 everywhere
@pytest.mark.parametrize("last_first,s0,want_nodes", [(False, 5, [3, 5, 6]), (True, 4, [3, 5, 7])])
def test_all_temperatures_zero_is_verify_tree(hip, params, truth, last_first, s0, want_nodes):
    """the two 7-draft trees of test_gpu_speculate_tree (non-first branch; page
    edge at 16 from position 13): acc, tokens and nodes are verify_tree's, the
    next steps the oracle's greedy stream, the K/V the oracle's"""
    trees = [_nonfirst(truth.stream[s0 + 1:s0 + 4, b], last_first=last_first) for b in range(B)]
    g = _model(hip, params, s0, truth.stream)
    want = g.verify_tree(trees)
    g.close()
    m = _model(hip, params, s0, truth.stream)
    _sampled(m, 99, [0.0] * B)
    acc, toks, nodes, probs = m.verify_tree_sampled(trees, want_probs=True)
    assert (acc, toks, nodes) == want and acc == [3] * B and nodes == [want_nodes] * B
    for b in range(B):  # point masses: 1 for the child that carries the greedy id of its parent's row
        ids, par = trees[b]
        on = [0] + nodes[b]
        for j in range(7):
            if par[j] in on:
                assert probs[b][j] == (1.0 if j + 1 in on else 0.0), (b, j)
    s = s0 + 4
    assert np.array_equal(_pending(hip, m), truth.stream[s])
    for t in range(12):
        assert np.array_equal(m.step(None), truth.stream[s + 1 + t]), t
    pos = m.positions()
    assert (pos == PRE + s + 12).all()
    worst = max(_kv_worst(m, lambda l, n, b=b: truth.orc.get_kv(l, b, n), b, int(pos[b])) for b in range(B))
    print(f"TREESPEC-S T = 0: worst K/V row ratio {worst:.3e} (bar {KV_RTOL[False]:.2e})")
    assert worst <= KV_RTOL[False]
    m.close()


# ---------------------------------------------------------------- 2. chains
@pytest.mark.parametrize("temps,seed", [(TEMPS, 39618), (LOW_TEMPS, 1001)])
def test_chain_shaped_trees_are_verify_sampled(hip, params, truth, temps, seed):
    s0, ks = 3, [7, 4, 2, 6]
    rng = np.random.default_rng(21)
    drafts = [truth.stream[s0 + 1:s0 + 1 + ks[b], b].copy() for b in range(B)]
    drafts[0][5] = rng.integers(0, V)
    drafts[1][1] = rng.integers(0, V)
    drafts[3][2] = (drafts[3][2] + 1) % V
    a = _model(hip, params, s0, truth.stream)
    _sampled(a, seed, temps)
    acc_c, toks_c, probs_c = a.verify_sampled([d.tolist() for d in drafts], want_probs=True)
    nxt_c = [a.step(None).tolist() for _ in range(2)]
    a.close()
    m = _model(hip, params, s0, truth.stream)
    _sampled(m, seed, temps)
    acc, toks, nodes, probs = m.verify_tree_sampled([(d.tolist(), list(range(len(d)))) for d in drafts],
                                                    want_probs=True)
    assert acc == acc_c and toks == toks_c
    assert nodes == [list(range(1, n + 1)) for n in acc]
    for b in range(B):
        assert probs[b].tobytes() == probs_c[b].tobytes(), b
    assert [m.step(None).tolist() for _ in range(2)] == nxt_c  # the same coin positions were reached
    m.close()


# ---------------------------------------------------------------- 3. branching under sampling
def _runner_up(x):
    return int(np.argsort(-x.astype(np.float64), kind="stable")[1])


def _branch_trees(truth_, s0):
    """per sequence, with t1, t2, t3 the next stream tokens, r1 the oracle's
    runner-up at the pending row, w a wrong id:
        r1(0) t1(0) w(2) t2(2) t3(4) x(1)
    -- the runner-up first and the greedy id second under the root, a wrong id
    ahead of the true one under t1, a leaf t3, and one off-stream node x under
    r1 (its row needs r1 fed)"""
    trees = []
    for b in range(B):
        t1, t2, t3 = (int(t) for t in truth_.stream[s0 + 1:s0 + 4, b])
        r1 = _runner_up(truth_.logits[s0, b])
        r2 = _runner_up(truth_.logits[s0 + 1, b])
        trees.append(([r1, t1, r2, t2, t3, (t2 + 7) % V], [0, 0, 2, 2, 4, 1]))
    return trees


def _node_rows(params_, truth_, s0, trees):
    """teacher-forced oracle logits of every internal node: its root path fed"""
    rows = [dict() for _ in range(B)]
    paths = []
    for b in range(B):
        ids, par = trees[b]
        internal = sorted({p for p in par})
        ps = []
        for node in internal:
            path, cur = [], node
            while cur:
                path.append(int(ids[cur - 1]))
                cur = par[cur - 1]
            ps.append((node, path[::-1]))
        paths.append(ps)
    for i in range(max(len(p) for p in paths)):
        fed = [[int(truth_.stream[s0, b])] + paths[b][min(i, len(paths[b]) - 1)][1] for b in range(B)]
        out = _teacher_forced(params_, [s0] * B, fed, truth_.stream)
        for b in range(B):
            rows[b][paths[b][min(i, len(paths[b]) - 1)][0]] = out[b][-1]
    return rows


def _plan(rows, trees, temps, seed, logit_tol):
    """From the oracle alone: per sequence the unconditional masses of every
    draft and their bounds, the coins, the walk (path, final node, rejected
    children there) -- asserting that every examined coin clears its bound."""
    out = []
    for b in range(B):
        ids, par = trees[b]
        T = temps[b]
        us = _coins(seed + b, len(ids) + 2)
        p64 = [_mass64(rows[b][par[j]], T, ids[j]) for j in range(len(ids))]
        eps = 2 * logit_tol / T if T > 0 else 0.0
        bound = [eps * p + (QUANTUM if p < QUANTUM else 0.0) if T > 0 else 0.0 for p in p64]
        cur, path, n_coin, events = 0, [], 0, []
        while True:
            s, rej, nxt = 0.0, [], None
            kids = ts.children(par, cur)
            for c in kids:
                p, u = p64[c - 1], float(us[n_coin])
                n_coin += 1
                if T == 0:
                    srt = np.sort(rows[b][cur])
                    assert srt[-1] - srt[-2] > 2 * logit_tol, ("greedy margin", b, cur)
                    q, bq = p, 0.0
                else:
                    q = p / (1 - s)
                    bq = 2 * eps * q * (1 + s / (1 - s)) + (QUANTUM if p < QUANTUM else 0.0)
                    assert abs(u - q) > bq, ("coin too close", b, c, u, q, bq)
                if u < q:
                    nxt = c
                    break
                s += p
                rej.append(int(ids[c - 1]))
            if nxt is None:
                break
            if rej:
                events.append("non-first")
            path.append(nxt)
            cur = nxt
        kids = ts.children(par, cur)
        events.append("leaf" if not kids else "all rejected of %d" % len(kids))
        out.append(dict(p64=p64, bound=bound, us=us, path=path, cur=cur, rej=rej, examined=n_coin, events=events))
    return out


# found by the search described in the module docstring (tools are not needed to
# rerun it: _plan asserts everything the test relies on)
TREE_TEMPS = [0.03, 0.05, 0.02, 0.0]
TREE_SEED = 6


def _assert_scenarios(plan, temps):
    ev = [set(p["events"]) for p in plan]
    assert any("non-first" in e and temps[b] > 0 for b, e in enumerate(ev)), ev
    assert any("all rejected of 2" in e for e in ev), ev
    assert any("leaf" in e for e in ev), ev


def test_branching_under_sampling(hip, params, truth):
    s0, temps, seed = 3, TREE_TEMPS, TREE_SEED
    trees = _branch_trees(truth, s0)
    rows = _node_rows(params, truth, s0, trees)
    plan = _plan(rows, trees, temps, seed, LOGIT_TOL)
    _assert_scenarios(plan, temps)
    m = _model(hip, params, s0, truth.stream)
    _sampled(m, seed, temps)
    pos0 = m.positions()
    acc, toks, nodes, probs = m.verify_tree_sampled(trees, want_probs=True)
    lg = m.logits()
    worst = 0.0
    for b in range(B):
        ids, par = trees[b]
        T, pl = temps[b], plan[b]
        for j in range(len(ids)):  # every draft, examined or not
            err = abs(float(probs[b][j]) - pl["p64"][j])
            worst = max(worst, err / pl["p64"][j] * T if pl["p64"][j] > QUANTUM and T > 0 else 0.0)
            assert err <= pl["bound"][j], (b, j, probs[b][j], pl["p64"][j], pl["bound"][j])
        assert nodes[b] == pl["path"] and acc[b] == len(pl["path"]), (b, nodes[b], pl["path"])  # decisions: exact
        assert toks[b][:-1] == [ids[c - 1] for c in pl["path"]]
        own, u_own = toks[b][-1], pl["us"][pl["examined"]]
        if T == 0:
            assert own == int(np.argmax(lg[b]))
        else:
            assert own not in pl["rej"], (b, own, pl["rej"])
            ts.check_pick_residual_multi(lg[b], T, V, lg[b].min(), pl["rej"], u_own, own, sr.tolerance(lg[b], T))
    print(f"TREESPEC-S branching: paths {nodes}, events {[p['events'] for p in plan]}, "
          f"worst relative probability error * T {worst:.3e} (bar {2 * LOGIT_TOL:.1e})")
    assert np.array_equal(m.positions(), pos0 + np.asarray(acc) + 1)
    assert np.array_equal(_pending(hip, m), [t[-1] for t in toks])
    # the accepted path's K/V (pending id and accepted drafts) against an oracle fed the same tokens
    c = oc.cfg(SMALL["maxT"], V, SMALL["L"], SMALL["NH"], SMALL["C"])
    pre = _forced()
    kv_worst = 0.0
    for b in range(B):
        o = oc.PagedDecoder(params, c, 1, P, SMALL["maxT"], page_seed=b + 1)
        for t in list(pre[:, b]) + list(truth.stream[:s0 + 1, b]) + toks[b][:-1]:
            o.step(np.array([t], np.int32))
        kv_worst = max(kv_worst, _kv_worst(m, lambda l, n: o.get_kv(l, 0, n), b, int(pos0[b]) + acc[b] + 1))
        o.close()
    print(f"TREESPEC-S branching: worst K/V row ratio {kv_worst:.3e} (bar {KV_RTOL[False]:.2e})")
    assert kv_worst <= KV_RTOL[False]
    # the next plain step draws coin number examined + 2
    nxt = m.step(None)
    lg = m.logits()
    for b in range(B):
        u = _coins(seed + b, plan[b]["examined"] + 2)[-1]
        sr.check_pick_any(lg[b], temps[b], 0, 1.0, u, int(nxt[b]), sr.tolerance(lg[b], temps[b]) if temps[b] else 0.0)
    m.close()


# ---------------------------------------------------------------- 4. n_draft -1 and 0
def test_untouched_sequences_and_plain_steps_match_a_twin(hip, params, truth):
    s0, seed, temps = 3, 77, [1.0, 0.7, 1.5, 1.0]
    tw = _model(hip, params, s0, truth.stream)
    _sampled(tw, seed, temps)
    m = _model(hip, params, s0, truth.stream)
    _sampled(m, seed, temps)
    pos0, pend0, lg0 = m.positions(), _pending(hip, m), m.logits()
    acc, toks, nodes, probs = m.verify_tree_sampled([None, ([], []), None, ([], [])], want_probs=True)
    step = tw.step(None)  # n_draft = 0 is a mode-2 step
    assert acc == [None, 0, None, 0] and toks[0] is None and nodes[2] is None and probs[0] is None
    assert [toks[1][0], toks[3][0]] == [int(step[1]), int(step[3])]
    pos, pend, lg = m.positions(), _pending(hip, m), m.logits()
    assert np.array_equal(pos, pos0 + [0, 1, 0, 1])
    for b in (0, 2):  # untouched: position, pending id, logits row
        assert pend[b] == pend0[b] and np.array_equal(lg[b].view(np.int32), lg0[b].view(np.int32))
    for b in (1, 3):  # the pass's row and the decode step's: each within LOGIT_TOL of the oracle's
        assert float(np.abs(lg[b] - tw.logits()[b]).max()) <= 2 * LOGIT_TOL
    acc2 = m.verify_tree_sampled([None] * B)[0]
    assert acc2 == [None] * B and np.array_equal(m.positions(), pos)
    # sampler states: sequences 0 and 2 draw their first coin now, 1 and 3 their second
    nxt = m.step(None)
    lg = m.logits()
    for b in range(B):
        u = _coins(seed + b, 2 if b in (1, 3) else 1)[-1]
        sr.check_pick(lg[b], temps[b], V, lg[b].min(), u, int(nxt[b]), sr.tolerance(lg[b], temps[b]))
    nxt_tw = tw.step(None)
    assert [int(nxt[1]), int(nxt[3])] == [int(nxt_tw[1]), int(nxt_tw[3])]
    m.close()
    tw.close()


# ---------------------------------------------------------------- 5. refusals
def _raw(hip, m, ids, parents, nd):
    ids = np.ascontiguousarray(ids, np.int32)
    parents = np.ascontiguousarray(parents, np.int32)
    nd = np.ascontiguousarray(nd, np.int32)
    acc = np.full(len(nd), -7, np.int32)
    toks = np.zeros((len(nd), MR), np.int32)
    nodes = np.zeros((len(nd), MR), np.int32)
    pr = np.zeros((len(nd), MR), np.float32)
    return hip.lib().gpt2_decode_verify_tree_sampled(m.h, ids.ctypes.data_as(_I), parents.ctypes.data_as(_I),
                                                     nd.ctypes.data_as(_I), acc.ctypes.data_as(_I),
                                                     toks.ctypes.data_as(_I), nodes.ctypes.data_as(_I),
                                                     pr.ctypes.data_as(_F))


def _state(hip, e):
    return (e.positions().tolist(), e.free_pages(), _pending(hip, e).tolist())


def test_refusals_change_nothing(hip, params, truth):
    """every refusal leaves positions, free pages, pending ids and sampler
    states as they were: afterwards the next step's tokens are a twin's"""
    seed = 3
    ok = truth.stream[1:4, 0]
    m = _prepared(hip, params)
    tw = _prepared(hip, params)
    s0 = _state(hip, m)
    assert _raw(hip, m, ok, [0, 1, 2], [3, 0, 0, 0]) != 0 and _state(hip, m) == s0   # mode 0: verify_tree's ground
    m.set_sampling(True, seed=seed, filtered=False)
    assert _raw(hip, m, ok, [0, 1, 2], [3, 0, 0, 0]) != 0 and _state(hip, m) == s0   # mode 1: no integer masses
    for e in (m, tw):
        e.set_sampling(True, seed=seed, filtered=True)
        e.set_sampling_params(-1, temperature=0.9)
    assert _raw(hip, m, ok, [0, 2, 1], [3, 0, 0, -1]) != 0 and _state(hip, m) == s0   # parent of draft 1 is 2 > 1
    assert _raw(hip, m, ok, [0, -1, 1], [3, 0, 0, -1]) != 0 and _state(hip, m) == s0  # parent < 0
    assert _raw(hip, m, [5, 6, 7, 5], [0, 0, 0, 0], [0, 4, 0, 0]) != 0 and _state(hip, m) == s0  # equal-token siblings
    assert _raw(hip, m, [5, V, 6], [0, 0, 0], [3, 0, 0, 0]) != 0 and _state(hip, m) == s0   # id == V
    assert _raw(hip, m, [5, -1, 6], [0, 0, 0], [3, 0, 0, 0]) != 0 and _state(hip, m) == s0  # id < 0
    assert _raw(hip, m, ok, [0, 1, 2], [8, 0, 0, 0]) != 0 and _state(hip, m) == s0    # n_draft > 7
    assert _raw(hip, m, ok, [0, 1, 2], [-2, 0, 0, 0]) != 0 and _state(hip, m) == s0   # n_draft < -1
    assert np.array_equal(m.step(None), tw.step(None))  # no coin was drawn, nothing moved
    m.close()
    tw.close()

    m = hip.Model(SMALL, params=params)  # max_ctx 16: position 9 + 8 rows overflows
    m.decode_init(B, P, 16)
    pre = _forced()
    for t in range(PRE):
        m.step(pre[t])
    m.set_sampling(True, seed=seed, filtered=True)
    s0 = _state(hip, m)
    seven = truth.stream[1:8, 0]
    assert _raw(hip, m, np.tile(seven, 4), np.tile(np.arange(7), 4), [7, 7, 7, 7]) != 0 and _state(hip, m) == s0
    m.close()

    p = _prepared(hip, params, processors=True)  # logit processors on
    p.set_sampling(True, seed=seed, filtered=True)
    sp_ = _state(hip, p)
    assert _raw(hip, p, ok, [0, 1, 2], [3, 0, 0, 0]) != 0 and _state(hip, p) == sp_
    p.close()

    h = _prepared(hip, params, kv_dtype=hip.HPA_BF16, w_dtype=hip.HPA_BF16)  # a bf16 pool: no tree mask there
    h.set_sampling(True, seed=seed, filtered=True)
    sh = _state(hip, h)
    assert hip.verify_plan(4, hip.HPA_BF16, P) == 0
    assert _raw(hip, h, ok, [0, 1, 2], [3, 0, 0, 0]) != 0 and _state(hip, h) == sh
    h.close()

    fresh = hip.Model(SMALL, params=params)  # no engine
    assert _raw(hip, fresh, ok, [0, 1, 2], [3, 0, 0, 0]) != 0
    fresh.close()


# ---------------------------------------------------------------- 6. the driver
def test_c_driver_at_temperature_zero_prints_the_greedy_ids(hip, params, truth, tmp_path):
    """examples/decode_main.c --speculate-tree-sampled 7 --temperature 0 against
    the greedy driver (-g): the same ids, and the closing lines of a tree run"""
    N = 40
    assert truth.margin[:N].min() > TIE_MARGIN
    libdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm.c-paged_amd")
    repo = os.path.dirname(libdir)
    exe = str(tmp_path / "decode_main")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", os.path.join(repo, "examples", "decode_main.c"),
                    "-I" + os.path.join(repo, "include"), "-L" + libdir, "-lpaged_hip", "-Wl,-rpath," + libdir,
                    "-o", exe], check=True)
    ck = str(tmp_path / "small.bin")
    synth.write_checkpoint(ck, SMALL, params)
    tok = tmp_path / "prompt.bin"
    np.ascontiguousarray(_forced().T).tofile(tok)
    outs = []
    for extra in (["-g"], ["--speculate-tree-sampled", "7", "--tree-depth", "3", "--temperature", "0"]):
        ids = tmp_path / f"ids{len(extra)}.bin"
        r = subprocess.run([exe, "-c", ck, "-t", str(tok), "-b", str(B), "-p", str(PRE), "-n", str(N), "-o", str(ids)]
                           + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append((np.fromfile(ids, np.int32).reshape(B, PRE + N), r.stdout))
    (plain, _), (spec, text) = outs
    assert np.array_equal(plain[:, PRE:], truth.stream[:N].T)
    assert np.array_equal(spec, plain)
    line = [ln for ln in text.splitlines() if ln.startswith("speculation:")]
    tree = [ln for ln in text.splitlines() if ln.startswith("tree speculation:")]
    assert len(line) == 1 and len(tree) == 1
    for bad in (["-g", "--speculate-tree-sampled", "4"], ["--speculate-tree-sampled", "8"],
                ["--speculate-tree-sampled", "4", "--speculate-tree", "4"],
                ["--speculate-tree-sampled", "4", "--ban", "5"]):
        r = subprocess.run([exe, "-c", ck, "-b", "1", "-p", "2", "-n", "2"] + bad, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "speculate" in r.stderr, bad
