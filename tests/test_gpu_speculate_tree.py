"""Engine-level tree speculation: gpt2_decode_verify_tree against the oracle's
token-by-token greedy stream, on the model, batch and truth of
tests/test_gpu_speculate.py (SMALL, B = 4, page 16, 9 forced tokens, then 64
greedy steps).

Ids are compared exactly under that module's own condition: the oracle's top-2
margin is >= MIN_MARGIN on every stream row (the `truth` fixture asserts it).
The accept walk only ever decides at nodes on the true stream -- it leaves a
node for a child only when that child carries the node's greedy id -- so no
further margin condition is needed.  Wrong siblings are (id + 1 + i) % V for
distinct i: they never equal the greedy id or each other.

Trees are written as (ids, parents): draft j is node j + 1 and hangs from node
parents[j] (node 0: the pending id).  With t1, t2, t3 the next three stream
tokens and w* wrong ids:

    non-first branch (7 drafts)   w(0) w(1) t1(0) w(3) t2(3) t3(5) w(5)
                                  accepted nodes 3, 5, 6
    page edge (7 drafts)          w(0) w(1) t1(0) w(3) t2(3) w(5) t3(5)
                                  accepted nodes 3, 5, 7
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc  # noqa: F401  (the truth fixture's decoder)
from test_gpu_kv_append import KV_RTOL
from test_gpu_score import LOGIT_TOL, SMALL, TIE_MARGIN, V
from test_gpu_speculate import B, MIN_MARGIN, P, PRE, STEPS, _Truth, _forced, _model, _pending

pytestmark = pytest.mark.gpu
MR = 8
_I = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def params():
    import synth
    return synth.params(SMALL, seed=11)


@pytest.fixture(scope="module")
def truth(params):
    t = _Truth(params)
    assert t.margin.min() >= MIN_MARGIN, t.margin.min()
    assert STEPS >= 32
    yield t
    t.close()


def _w(tok, i=0):
    return int((int(tok) + 1 + i) % V)


def _nonfirst(t, last_first=False):
    """the 7-draft tree of the module docstring around the true tokens t[0..2];
    last_first: t3 is node 7 and its wrong sibling node 6"""
    t1, t2, t3 = (int(x) for x in t)
    tail = [_w(t3), t3] if last_first else [t3, _w(t3)]
    return [_w(t1), _w(t2), t1, _w(t2), t2] + tail, [0, 1, 0, 3, 3, 5, 5]


def test_true_stream_on_a_non_first_branch(hip, params, truth):
    """depth 3, 7 drafts, the true continuation behind wrong siblings at every
    depth: accepted nodes 3, 5, 6; tokens, positions, pending id and the logits
    row are those of 4 greedy steps"""
    s0 = 5
    m = _model(hip, params, s0, truth.stream)
    trees = [_nonfirst(truth.stream[s0 + 1:s0 + 4, b]) for b in range(B)]
    pos0 = m.positions()
    acc, toks, nodes = m.verify_tree(trees)
    assert acc == [3] * B
    for b in range(B):
        assert toks[b] == truth.stream[s0 + 1:s0 + 5, b].tolist(), b
        assert nodes[b] == [3, 5, 6], b
    assert np.array_equal(m.positions(), pos0 + 4)
    assert np.array_equal(_pending(hip, m), truth.stream[s0 + 4])
    d = float(np.abs(m.logits() - truth.logits[s0 + 4]).max())
    print(f"TREESPEC non-first branch: worst |logit diff| {d:.3e} (bar {LOGIT_TOL:.1e})")
    assert d <= LOGIT_TOL
    for t in range(3):  # decoding goes on from the compacted state
        assert np.array_equal(m.step(None), truth.stream[s0 + 5 + t]), t
    m.close()


@pytest.mark.parametrize("j", [0, 1, 2])
def test_branch_switch(hip, params, truth, j):
    """the first branch is a chain of 3 that is true for j tokens and wrong
    from there; the true continuation hangs off its node j, to depth 3"""
    s0 = 6
    m = _model(hip, params, s0, truth.stream)
    trees, want = [], []
    for b in range(B):
        t = [int(x) for x in truth.stream[s0 + 1:s0 + 4, b]]
        ids = [t[i] if i < j else _w(t[i], b) for i in range(3)]
        par = [0, 1, 2]
        path = list(range(1, j + 1))
        cur = j
        for i in range(j, 3):  # the true tokens from depth j on, appended after the first branch
            ids.append(t[i])
            par.append(cur)
            cur = len(ids)
            path.append(cur)
        trees.append((ids, par))
        want.append(path)
    pos0 = m.positions()
    acc, toks, nodes = m.verify_tree(trees)
    assert acc == [3] * B and nodes == want
    for b in range(B):
        assert toks[b] == truth.stream[s0 + 1:s0 + 5, b].tolist(), b
    assert np.array_equal(m.positions(), pos0 + 4)
    assert np.array_equal(_pending(hip, m), truth.stream[s0 + 4])
    assert float(np.abs(m.logits() - truth.logits[s0 + 4]).max()) <= LOGIT_TOL
    m.close()


def test_no_child_matches(hip, params, truth):
    """a star of 7 wrong ids (and shorter ones): a = 0, the result a plain decode step's"""
    s0 = 3
    m = _model(hip, params, s0, truth.stream)
    ks = [7, 3, 1, 7]
    trees = [([_w(truth.stream[s0 + 1, b], i) for i in range(ks[b])], [0] * ks[b]) for b in range(B)]
    pos0 = m.positions()
    acc, toks, nodes = m.verify_tree(trees)
    assert acc == [0] * B and nodes == [[]] * B
    assert [t[0] for t in toks] == truth.stream[s0 + 1].tolist()
    assert np.array_equal(m.positions(), pos0 + 1)
    assert np.array_equal(_pending(hip, m), truth.stream[s0 + 1])
    assert float(np.abs(m.logits() - truth.logits[s0 + 1]).max()) <= LOGIT_TOL
    assert np.array_equal(m.step(None), truth.stream[s0 + 2])
    m.close()


def test_page_edge_then_decode_on(hip, params, truth):
    """a pass from position 13 (page edge at 16) whose accepted path is nodes
    3, 5, 7: sources in slots 16, 18, 20 of the next page, destinations 14, 15,
    16 across the edge.  Then 12 decode steps and the K/V of every position and
    layer against the oracle's: a wrong wpe position (depth, not node index) or
    a wrong compaction shows here"""
    s0 = 4
    m = _model(hip, params, s0, truth.stream)
    assert (m.positions() == 13).all()
    trees = [_nonfirst(truth.stream[s0 + 1:s0 + 4, b], last_first=True) for b in range(B)]
    acc, toks, nodes = m.verify_tree(trees)
    assert acc == [3] * B and nodes == [[3, 5, 7]] * B
    s = s0 + 4
    assert np.array_equal(_pending(hip, m), truth.stream[s])
    for t in range(12):
        assert np.array_equal(m.step(None), truth.stream[s + 1 + t]), t
    pos = m.positions()
    assert (pos == PRE + s + 12).all()
    worst = 0.0
    for l in range(SMALL["L"]):
        for b in range(B):
            k, v = m.read_kv(l, b, int(pos[b]))
            ko, vo = truth.orc.get_kv(l, b, int(pos[b]))
            for got, ref in ((k, ko), (v, vo)):
                r = np.abs(got.astype(np.float64) - ref).max(-1) / np.abs(ref).max(-1)
                worst = max(worst, float(r.max()))
    print(f"TREESPEC page edge: worst K/V row ratio {worst:.3e} (bar {KV_RTOL[False]:.2e})")
    assert worst <= KV_RTOL[False]
    m.close()


def test_chain_shaped_tree_equals_the_chain_pass(hip, params, truth):
    """parents[j] = j: n_accepted, tokens and positions equal
    gpt2_decode_verify's on an identically prepared engine, and the logits row
    bit for bit (same kernels, same masks, the compaction a no-op)"""
    s0 = 5
    ks = [7, 3, 7, 1]
    drafts = [truth.stream[s0 + 1:s0 + 1 + ks[b], b].copy() for b in range(B)]
    drafts[0][4] = _w(drafts[0][4])  # one rejection in the middle of a chain
    a = _model(hip, params, s0, truth.stream)
    acc_c, toks_c, _ = a.verify([d.tolist() for d in drafts])
    lg_c, pos_c = a.logits(), a.positions()
    a.close()
    m = _model(hip, params, s0, truth.stream)
    acc_t, toks_t, nodes = m.verify_tree([(d.tolist(), list(range(len(d)))) for d in drafts])
    assert acc_t == acc_c == [4, 3, 7, 1] and toks_t == toks_c
    assert nodes == [list(range(1, n + 1)) for n in acc_t]
    assert np.array_equal(m.positions(), pos_c)
    assert np.array_equal(m.logits().view(np.int32), lg_c.view(np.int32))
    m.close()


def test_untouched_sequences(hip, params, truth):
    """None rows: position, pending id and logits row (bitwise) unchanged
    beside advancing ones; all untouched: nothing moves"""
    s0 = 3
    m = _model(hip, params, s0, truth.stream)
    pos0, pend0, lg0 = m.positions(), _pending(hip, m), m.logits()
    trees = [_nonfirst(truth.stream[s0 + 1:s0 + 4, 0]), None, ([], []), None]
    acc, toks, nodes = m.verify_tree(trees)
    assert acc == [3, None, 0, None] and toks[1] is None and nodes[3] is None and nodes[2] == []
    assert toks[0] == truth.stream[s0 + 1:s0 + 5, 0].tolist() and toks[2] == [int(truth.stream[s0 + 1, 2])]
    pos, pend, lg = m.positions(), _pending(hip, m), m.logits()
    assert np.array_equal(pos, pos0 + [4, 0, 1, 0])
    for b in (1, 3):
        assert pend[b] == pend0[b] and np.array_equal(lg[b].view(np.int32), lg0[b].view(np.int32))
    assert pend[0] == truth.stream[s0 + 4, 0] and pend[2] == truth.stream[s0 + 1, 2]
    free0 = m.free_pages()
    acc, toks, nodes = m.verify_tree([None] * B)
    assert acc == [None] * B and np.array_equal(m.positions(), pos) and m.free_pages() == free0
    assert np.array_equal(_pending(hip, m), pend) and np.array_equal(m.logits().view(np.int32), lg.view(np.int32))
    nxt = m.step(None)
    assert nxt[1] == truth.stream[s0 + 1, 1] and nxt[0] == truth.stream[s0 + 5, 0]
    m.close()


def _raw(hip, m, ids, parents, nd):
    ids = np.ascontiguousarray(ids, np.int32)
    parents = np.ascontiguousarray(parents, np.int32)
    nd = np.ascontiguousarray(nd, np.int32)
    acc = np.full(len(nd), -7, np.int32)
    toks = np.zeros((len(nd), MR), np.int32)
    nodes = np.zeros((len(nd), MR), np.int32)
    return hip.lib().gpt2_decode_verify_tree(m.h, ids.ctypes.data_as(_I), parents.ctypes.data_as(_I),
                                             nd.ctypes.data_as(_I), acc.ctypes.data_as(_I), toks.ctypes.data_as(_I),
                                             nodes.ctypes.data_as(_I))


def _prepared(hip, params, processors=False, **kw):
    m = hip.Model(SMALL, params=params)
    m.decode_init(B, P, SMALL["maxT"], **kw)
    if processors:
        m.set_processors(True)
    pre = _forced()
    for t in range(PRE):
        m.step(pre[t])
    return m


def test_refusals_change_nothing(hip, params, truth):
    """each refusal leaves positions, free pages and pending ids as they were"""
    m = _prepared(hip, params)
    state0 = (m.positions().tolist(), m.free_pages(), _pending(hip, m).tolist())

    def unchanged(e=m, s=state0):
        return (e.positions().tolist(), e.free_pages(), _pending(hip, e).tolist()) == s

    ok = truth.stream[1:4, 0]
    assert _raw(hip, m, ok, [0, 2, 1], [3, 0, 0, -1]) != 0 and unchanged()            # parent of draft 1 is 2 > 1
    assert _raw(hip, m, ok, [0, -1, 1], [3, 0, 0, -1]) != 0 and unchanged()           # parent < 0
    assert _raw(hip, m, [5, 6, 7, 5], [0, 0, 0, 0], [0, 4, 0, 0]) != 0 and unchanged()  # siblings 0 and 3: token 5
    assert _raw(hip, m, [5, 6, 6], [0, 1, 1], [0, 0, 3, -1]) != 0 and unchanged()     # siblings under node 1
    assert _raw(hip, m, [5, V, 6], [0, 0, 0], [3, 0, 0, 0]) != 0 and unchanged()      # id == V
    assert _raw(hip, m, ok, [0, 1, 2], [8, 0, 0, 0]) != 0 and unchanged()             # n_draft > 7
    for filtered in (False, True):                                                    # sampling modes 1 and 2
        m.set_sampling(True, seed=3, filtered=filtered)
        assert _raw(hip, m, ok, [0, 1, 2], [3, 0, 0, 0]) != 0 and unchanged(), filtered
    m.set_sampling(False)
    assert _raw(hip, m, [5, 6, 5], [0, 0, 1], [3, 0, 0, -1]) == 0  # the same token under different parents is fine
    assert m.positions().tolist()[3] == state0[0][3]
    m.close()

    p = _prepared(hip, params, processors=True)                                       # processors on
    sp = (p.positions().tolist(), p.free_pages(), _pending(hip, p).tolist())
    assert _raw(hip, p, ok, [0, 1, 2], [3, 0, 0, 0]) != 0 and unchanged(p, sp)
    p.close()

    h = _prepared(hip, params, kv_dtype=hip.HPA_BF16, w_dtype=hip.HPA_BF16)           # a bf16 pool: no tree mask there
    sh = (h.positions().tolist(), h.free_pages(), _pending(hip, h).tolist())
    assert hip.verify_plan(4, hip.HPA_BF16, P) == 0
    assert _raw(hip, h, ok, [0, 1, 2], [3, 0, 0, 0]) != 0 and unchanged(h, sh)
    assert _raw(hip, h, ok, [0, 1, 2], [0, 0, 0, 0]) != 0 and unchanged(h, sh)        # even without a draft
    h.close()


def test_c_driver_speculate_tree_prints_the_same_ids(hip, params, truth, tmp_path):
    """examples/decode_main.c -g with and without --speculate-tree 7 on a
    checkpoint of the small model, the forced tokens as the prompt, 40 new
    tokens: the same ids (the oracle's stream) and two closing lines more"""
    import synth
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
    np.ascontiguousarray(_forced().T).tofile(tok)  # (B, PRE): sequence-major
    outs = []
    for extra in ([], ["--speculate-tree", "7", "--tree-depth", "3"]):
        ids = tmp_path / f"ids{len(extra)}.bin"
        r = subprocess.run([exe, "-c", ck, "-t", str(tok), "-b", str(B), "-p", str(PRE), "-n", str(N), "-g",
                            "-o", str(ids)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append((np.fromfile(ids, np.int32).reshape(B, PRE + N), r.stdout))
    (plain, text0), (spec, text1) = outs
    assert np.array_equal(plain[:, PRE:], truth.stream[:N].T)
    assert np.array_equal(spec, plain)
    line = [ln for ln in text1.splitlines() if ln.startswith("speculation:")]
    tree = [ln for ln in text1.splitlines() if ln.startswith("tree speculation:")]
    assert len(line) == 1 and len(tree) == 1 and "speculation:" not in text0
    passes, tokens = int(line[0].split()[1]), int(line[0].split()[3])
    assert tokens == B * (N - 1) and passes < N - 1, line
    off, pairs = int(tree[0].split()[2]), int(tree[0].split()[4])
    assert 0 <= off <= pairs and pairs >= passes, tree
    for bad in (["--speculate-tree", "4"], ["-g", "--speculate-tree", "4", "--top-k", "5"],
                ["-g", "--speculate-tree", "8"], ["-g", "--speculate-tree", "4", "--speculate", "2"],
                ["-g", "--speculate-tree", "4", "--ban", "5"]):
        r = subprocess.run([exe, "-c", ck, "-b", "1", "-p", "2", "-n", "2"] + bad, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "speculate" in r.stderr, bad
