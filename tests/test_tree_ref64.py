"""Tree speculation without a GPU: the restatement of tests/tree_ref64.py
checked against itself (masks, depths, the accept walk), the in-place K/V
compaction against the out-of-place gather over EVERY tree of 1..7 drafts and
every root-to-node path, and the host drafter gpt2_ngram_draft_tree against
its restatement -- through the library, and compiled with a stand-alone main
under -fsanitize=address,undefined.

gpt2_decode_verify_tree validates its arguments against an engine's state, and
an engine needs a device: its refusals are in tests/test_gpu_speculate_tree.py;
here only the call without a model."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import pagedattn as pa
import tree_ref64 as tr
from test_verify_host import ngram_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_I = ctypes.POINTER(ctypes.c_int)


# ---------------------------------------------------------------- masks, depths, the walk
def test_masks_and_depths_of_the_named_shapes():
    assert tr.depths(tr.STAR).tolist() == [0, 1, 1, 1, 1, 1, 1, 1]
    assert tr.anc_masks(tr.STAR).tolist() == [1] + [1 | (1 << i) for i in range(1, 8)]
    assert tr.depths(tr.CHAIN).tolist() == list(range(8))
    assert tr.anc_masks(tr.CHAIN).tolist() == [(2 << i) - 1 for i in range(8)]  # the causal mask of a chain pass
    assert tr.depths(tr.TWO_CHAINS).tolist() == [0, 1, 2, 3, 1, 2, 3]
    assert tr.anc_masks(tr.TWO_CHAINS).tolist() == [1, 3, 7, 15, 0x11, 0x31, 0x71]
    assert tr.depths(tr.BINARY).tolist() == [0, 1, 1, 2, 2, 2, 2, 3]
    assert tr.anc_masks(tr.BINARY).tolist() == [1, 3, 5, 0b1011, 0b10011, 0b100101, 0b1000101, 0b10001011]


def test_mask_properties_over_every_tree():
    """own bit the highest, root always seen, popcount = depth + 1, and a
    node's mask is its parent's plus its own bit"""
    count = 0
    for nd in range(1, 8):
        for parents in tr.all_parent_arrays(nd):
            m, d = tr.anc_masks(parents), tr.depths(parents)
            for r in range(nd + 1):
                assert int(m[r]).bit_length() == r + 1 and m[r] & 1
                assert bin(int(m[r])).count("1") == d[r] + 1
                if r:
                    assert int(m[r]) == int(m[parents[r - 1]]) | (1 << r)
            count += 1
    assert count == sum(np.prod(np.arange(1, n + 1)) for n in range(1, 8))  # 5040 trees at 7 drafts


def test_accept_walk_named_cases():
    par = tr.TWO_CHAINS
    tok = [10, 20, 21, 22, 30, 31, 32]
    # the model follows the second branch to its end
    assert tr.accept(tok, [30, 0, 0, 0, 31, 32, 99], par) == [4, 5, 6]
    # leaves it after one node; the first branch's node 2 carries the id but hangs elsewhere
    assert tr.accept(tok, [30, 0, 0, 0, 21, 0, 0], par) == [4]
    # first branch, two deep
    assert tr.accept(tok, [20, 21, 7, 0, 0, 0, 0], par) == [1, 2]
    # no child of the root matches
    assert tr.accept(tok, [21, 21, 22, 0, 31, 32, 0], par) == []
    # duplicate siblings (refused by the engine): the lower index wins
    assert tr.accept([1, 5, 5], [5, 0, 0], [0, 0]) == [1]


# ---------------------------------------------------------------- compaction, exhaustively
def test_in_place_compaction_equals_the_gather_for_every_tree_and_path():
    """slot k <- slot path[k-1] walked in ascending k on the live array equals
    the out-of-place gather, for every parent array of 1..7 drafts and every
    root-to-node path; walking k downwards does not"""
    slots = np.arange(100, 108)
    trees = checked = caught = 0
    for nd in range(1, 8):
        for parents in tr.all_parent_arrays(nd):
            trees += 1
            for path in tr.paths(parents):
                assert all(b > a for a, b in zip(path, path[1:])) and all(p >= k for k, p in enumerate(path, 1))
                want = tr.compact_gather(slots, path)
                assert np.array_equal(tr.compact_in_place(slots, path), want), (parents, path)
                caught += not np.array_equal(tr.compact_in_place(slots, path, descending=True), want)
                checked += 1
    assert trees == 1 + 2 + 6 + 24 + 120 + 720 + 5040
    print(f"TREE compaction: {trees} trees, {checked} paths, the descending mutant wrong on {caught}")
    assert caught > 0
    # a named case of the mutant: path (2, 3) -- slot 2 is destination of k = 2 and source of k = 1
    assert tr.compact_in_place(slots, [2, 3], descending=True).tolist()[:3] == [100, 103, 103]
    assert tr.compact_gather(slots, [2, 3]).tolist()[:3] == [100, 102, 103]


# ---------------------------------------------------------------- the drafter
GRID = [(mx, mn, nodes, depth, br) for mx in (1, 2, 3, 4) for mn in (1, 2) if mn <= mx
        for nodes in (1, 3, 4, 7) for depth in (1, 2, 4, 7) for br in (1, 2, 3, 7)]


def test_ngram_draft_tree_matches_the_restatement_on_random_histories():
    rng = np.random.default_rng(0)
    hits = branched = 0
    for mx, mn, nodes, depth, br in GRID:
        for _ in range(12):
            n = int(rng.integers(0, 40))
            h = rng.integers(0, int(rng.integers(2, 7)), n)
            ids, par = pa.ngram_draft_tree(h, nodes, depth, br, mx, mn)
            assert (ids, par) == tr.ngram_tree_ref(h, mx, mn, nodes, depth, br), (h.tolist(), mx, mn, nodes, depth, br)
            assert len(ids) <= nodes and tr.valid(par, ids), (ids, par)
            assert (tr.depths(par) <= depth).all()
            chain = ngram_ref(h, depth, mx, mn)  # gpt2_ngram_draft's restatement; checked against the library below
            assert chain == pa.ngram_draft(h, depth, mx, mn)
            assert bool(ids) == bool(chain)
            k = min(len(chain), nodes)  # depth > max_nodes: the first insertion is cut there
            assert tr.first_child_chain(ids, par)[:k] == chain[:k], (h.tolist(), ids, par, chain)
            hits += bool(ids)
            branched += len(set(par)) < len(par)
    print(f"TREE drafter: {len(GRID) * 12} histories, {hits} with a draft, {branched} with a branching node")
    assert hits > len(GRID) * 6 and branched > len(GRID)


def test_ngram_draft_tree_named_cases():
    h = [1, 2, 3, 1, 2, 4, 1, 2, 5, 1, 2]
    # "1 2" occurred three times: 5 (then 1 2), 4 (then 1 2 5), 3 (then 1 2 4): most recent first
    assert pa.ngram_draft_tree(h, 7, 4, 3) == ([5, 1, 2, 4, 1, 2, 5], [0, 1, 2, 0, 4, 5, 6])
    assert pa.ngram_draft_tree(h, 7, 2, 3) == ([5, 1, 4, 1, 3, 1], [0, 1, 0, 3, 0, 5])
    assert pa.ngram_draft_tree(h, 7, 1, 7) == ([5, 4, 3], [0, 0, 0])
    assert pa.ngram_draft_tree(h, 7, 1, 2) == ([5, 4], [0, 0])        # max_branches
    assert pa.ngram_draft_tree(h, 2, 1, 7) == ([5, 4], [0, 0])        # max_nodes
    assert pa.ngram_draft_tree(h, 4, 4, 3) == ([5, 1, 2, 4], [0, 1, 2, 0])  # the second insertion cut at max_nodes
    # shared prefixes: both occurrences of "7" go on with 8, then differ (8 2 7 and 8 1 7)
    assert pa.ngram_draft_tree([7, 8, 1, 7, 8, 2, 7], 7, 3, 3, 1, 1) == ([8, 2, 7, 1, 7], [0, 1, 2, 1, 4])
    # no match, bad arguments
    assert pa.ngram_draft_tree([1, 2, 3, 4]) == ([], [])
    assert pa.ngram_draft_tree([], 7) == ([], [])
    for bad in (dict(max_nodes=0), dict(max_nodes=8), dict(depth=0), dict(max_branches=0), dict(min_ngram=0)):
        assert pa.ngram_draft_tree(h, **bad) == ([], []), bad


_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int gpt2_ngram_draft(const int* history, int n, int max_ngram, int min_ngram, int k, int* draft);
int gpt2_ngram_draft_tree(const int* history, int n, int max_ngram, int min_ngram, int max_nodes, int depth,
                          int max_branches, int* draft, int* parents);

int main(void) {
    unsigned long long st = 88172645463325252ull;
    long hits = 0, branched = 0;
    for (int it = 0; it < 20000; it++) {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        const int n = (int)(st % 48), nodes = (int)((st >> 8) % 9), mx = 1 + (int)((st >> 16) % 5);
        const int mn = 1 + (int)((st >> 24) % (unsigned)mx), depth = (int)((st >> 32) % 9);
        const int br = (int)((st >> 40) % 5), alpha = 2 + (int)((st >> 48) % 5);
        /* exact-size heap blocks: any read or write past them is reported */
        const int room = nodes >= 1 && nodes <= 7 ? nodes : 1;
        int* h = (int*)malloc((size_t)(n ? n : 1) * sizeof(int));
        int* ids = (int*)malloc((size_t)room * sizeof(int));
        int* par = (int*)malloc((size_t)room * sizeof(int));
        int* chain = (int*)malloc((size_t)(depth > 0 ? depth : 1) * sizeof(int));
        unsigned long long s2 = st;
        for (int i = 0; i < n; i++) { s2 = s2 * 6364136223846793005ull + 1442695040888963407ull; h[i] = (int)((s2 >> 33) % (unsigned)alpha); }
        const int nd = gpt2_ngram_draft_tree(h, n, mx, mn, nodes, depth, br, ids, par);
        if (nd < 0 || nd > room || (nd && (nodes < 1 || nodes > 7 || depth < 1 || br < 1))) { printf("COUNT at %d\n", it); return 1; }
        int forks = 0;
        for (int j = 0; j < nd; j++) {
            if (par[j] < 0 || par[j] > j) { printf("PARENT at %d\n", it); return 1; }
            for (int i = 0; i < j; i++) {
                if (par[i] == par[j] && ids[i] == ids[j]) { printf("SIBLINGS at %d\n", it); return 1; }
                forks |= par[i] == par[j];
            }
        }
        /* the first-child chain is the chain drafter's draft (cut at max_nodes) */
        if (nodes >= 1 && nodes <= 7 && depth >= 1 && br >= 1) {
            const int nc = gpt2_ngram_draft(h, n, mx, mn, depth, chain);
            if ((nc > 0) != (nd > 0)) { printf("MATCH at %d\n", it); return 1; }
            int cur = 0;
            for (int i = 0; i < nc && i < nodes; i++) {
                int c = -1;
                for (int j = 0; j < nd && c < 0; j++) if (par[j] == cur) c = j;
                if (c < 0 || ids[c] != chain[i]) { printf("CHAIN at %d\n", it); return 1; }
                cur = c + 1;
            }
        }
        hits += nd > 0;
        branched += forks;
        free(h); free(ids); free(par); free(chain);
    }
    printf("NGRAM_TREE_SAN ok hits=%ld branched=%ld\n", hits, branched);
    return hits > 4000 && branched > 1000 ? 0 : 2;
}
"""


def test_ngram_draft_tree_standalone_under_asan_ubsan(tmp_path):
    """csrc/ngram_draft.c and a stand-alone main, both under
    -fsanitize=address,undefined: 20000 random histories in exact-size heap
    buffers; every tree well formed and its first-child chain the chain draft"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    fn = os.path.join(REPO, "llm.c-paged_amd", "csrc", "ngram_draft.c")
    main = tmp_path / "main.c"
    main.write_text(_MAIN)
    exe = tmp_path / "ngram_tree_san"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run([cc, *flags, str(fn), str(main), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "NGRAM_TREE_SAN ok" in r.stdout


def test_verify_tree_without_an_engine_is_refused():
    """no model / no engine: nonzero before anything is read"""
    L = pa.lib()
    one = (ctypes.c_int * 8)()
    assert L.gpt2_decode_verify_tree(None, one, one, one, one, one, None) != 0
