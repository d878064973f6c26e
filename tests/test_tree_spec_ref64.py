"""Sampled tree speculation without a GPU: the rule's exactness in exact
fractions (the coins integrated out analytically, nothing sampled), the
integer walk against spec_ref64.accept_walk on chains and against the rational
comparison at its edges, and the pure host function gpt2_tree_dense_tables
against its restatement -- through ctypes, and compiled with a small
stand-alone main under -fsanitize=address,undefined and run."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np

import pagedattn as pa
import sample_ref64 as sr
import spec_ref64 as sp
import tree_ref64 as tr
import tree_spec_ref64 as ts

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dist(rng, V, zeros=0):
    """a random distribution over V tokens in exact fractions, `zeros` of them with no mass"""
    w = [int(x) for x in rng.integers(1, 1000, V)]
    for i in rng.choice(V, zeros, replace=False):
        w[int(i)] = 0
    s = sum(w)
    return {i: Fraction(w[i], s) for i in range(V)}


def _sibling_tokens(rng, parents, V):
    """random ids, distinct among siblings"""
    ids = []
    for j, p in enumerate(parents):
        taken = {ids[i] for i in range(j) if parents[i] == p}
        ids.append(int(rng.choice([t for t in range(V) if t not in taken])))
    return ids


# ---------------------------------------------------------------- exactness
def test_first_emitted_token_is_distributed_as_p_for_every_tree_shape():
    rng = np.random.default_rng(17)
    shapes = 0
    for n in range(0, 5):
        for parents in tr.all_parent_arrays(n):
            V = int(rng.integers(6, 13))
            p = _dist(rng, V, zeros=int(rng.integers(0, 3)))
            ids = _sibling_tokens(rng, parents, V)
            root_kids = [ids[c - 1] for c in ts.children(parents, 0)]
            law = ts.first_law(p, root_kids)
            assert law == {k: v for k, v in p.items() if v > 0}, (parents, ids)
            shapes += 1
    assert shapes == 1 + 1 + 2 + 6 + 24


def test_first_two_emitted_tokens_follow_the_product_law():
    rng = np.random.default_rng(23)
    for n in range(1, 5):
        for parents in tr.all_parent_arrays(n):
            V = int(rng.integers(6, 9))
            memo = {}

            def table(prefix):
                if prefix not in memo:
                    memo[prefix] = _dist(rng, V, zeros=int(rng.integers(0, 3)))
                return memo[prefix]

            ids = _sibling_tokens(rng, parents, V)
            got = ts.emitted_law(table, ids, list(parents), (), 2)
            want = ts.plain_law(table, (), 2)
            assert got == want, (parents, ids)
            assert sum(got.values()) == 1


# ---------------------------------------------------------------- the integer walk
def test_walk_on_chains_is_the_chain_walk():
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        n = int(rng.integers(0, 8))
        ws = [int(x) for x in rng.integers(1, 1 << 62, n, dtype=np.uint64)]
        wt = [int(w * f) if f < 1 else w for w, f in zip(ws, rng.choice([0.0, 0.3, 0.9, 1.0], n))]
        drafts = rng.integers(0, 50257, n).tolist()
        seed = int(rng.integers(1, 1 << 63, dtype=np.uint64))
        st, a, rej, coins = sp.accept_walk(seed, wt, ws, drafts)
        st2, path, cur, rejs, coins2, _ = ts.walk(seed, wt, ws, drafts, list(range(n)))
        assert (st2, len(path), cur, coins2) == (st, a, a, coins)
        assert path == list(range(1, a + 1))
        assert rejs == ([] if rej < 0 else [rej])
        seen.add("all" if rej < 0 else "some")
    assert seen == {"all", "some"}


def test_walk_advances_once_per_examined_child_and_rem_stays_positive():
    rng = np.random.default_rng(6)
    for _ in range(300):
        n = 7
        parents = [int(rng.integers(0, j + 1)) for j in range(n)]
        S = {node: int(rng.integers(1 << 20, 1 << 60)) for node in range(n + 1)}
        wt, ws = [0] * n, [0] * n
        for node in range(n + 1):
            kids = ts.children(parents, node)
            cutp = sorted(int(x) for x in rng.integers(0, S[node] + 1, len(kids)))
            left = S[node]
            for c, hi in zip(kids, cutp):  # disjoint masses: distinct tokens of one distribution
                w = min(left, hi // max(len(kids), 1))
                wt[c - 1], ws[c - 1] = w, S[node]
                left -= w
        seed = int(rng.integers(1, 1 << 63, dtype=np.uint64))
        st, path, cur, rej, coins, rem = ts.walk(seed, wt, ws, list(range(100, 100 + n)), parents)
        s = seed
        for _ in coins:
            s, _r = sr.xorshift_u32(s)
        assert s == st
        assert rem is None or rem > 0
        assert len(rej) <= len(ts.children(parents, cur))
        assert all(parents[c - 1] == p for p, c in zip([0] + path, path))


def test_integer_test_is_the_rational_comparison_at_the_edges():
    top = (1 << 24) - 1
    for rem in (1, 2, 3, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 44) + 12345, (1 << 62) - 1):
        for w in {0, 1, rem // 2, rem - 1, rem}:
            for j in (0, 1, top // 2, top - 1, top):
                assert ts.accepts(w, rem, j) == (Fraction(j, 1 << 24) < Fraction(w, rem)), (w, rem, j)
        assert all(ts.accepts(rem, rem, j) for j in (0, top))  # the whole remaining set: always accepted
        assert not any(ts.accepts(0, rem, j) for j in (0, top))  # no mass: never, not even at u = 0
    # a temperature-0 row: (1, 1) accepts at every coin, (0, 1) at none
    assert ts.accepts(1, 1, top) and not ts.accepts(0, 1, 0)


# ---------------------------------------------------------------- gpt2_tree_dense_tables
def _tables_case(rng, trees):
    B = len(trees)
    nd = np.array([-1 if t is None else len(t[0]) for t in trees])
    row0 = np.cumsum(nd + 1) - (nd + 1) + 3  # any base: the function only adds to it
    got = pa.tree_dense_tables(trees, row0)
    rows, seq, tg, nt, dst = ts.dense_tables(trees, row0)
    assert got[0].tolist() == rows and got[1].tolist() == seq and got[3].tolist() == nt, (trees,)
    assert got[2].tolist() == tg and got[4].tolist() == dst, (trees,)
    n_drafts = int(np.maximum(nd, 0).sum())
    assert len(rows) <= n_drafts
    # every draft is asked about exactly once, at its parent's row
    flat = sorted(d for row in dst for d in row if d >= 0)
    assert flat == list(range(n_drafts))
    return B


def test_dense_tables_match_the_restatement_over_every_small_tree():
    rng = np.random.default_rng(31)
    for n in range(0, 6):
        for parents in tr.all_parent_arrays(n):
            ids = _sibling_tokens(rng, parents, 50)
            trees = [None, (ids, list(parents)), ([], []), (ids, list(parents))]
            _tables_case(rng, trees)


def test_dense_tables_on_random_seven_draft_trees_and_a_star():
    rng = np.random.default_rng(32)
    for _ in range(200):
        trees = []
        for b in range(int(rng.integers(1, 6))):
            kind = int(rng.integers(0, 4))
            if kind == 0:
                trees.append(None)
            elif kind == 1:
                trees.append(([], []))
            else:
                parents = [int(rng.integers(0, j + 1)) for j in range(7)]
                trees.append((_sibling_tokens(rng, parents, 50), parents))
        _tables_case(rng, trees)
    rows, seq, tg, nt, dst = pa.tree_dense_tables([(list(range(10, 17)), tr.STAR)])
    assert rows.tolist() == [0] and nt.tolist() == [7]  # seven children, one dense row
    assert tg.tolist() == [list(range(10, 17))] and dst.tolist() == [list(range(7))]


_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int gpt2_tree_dense_tables(const int* drafts, const int* parents, const int* n_draft, int B, const int* row0, int* rows,
                           int* seq, int* targets, int* n_targets, int* dst);

int main(void) {
    unsigned long long st = 88172645463325252ull;
    long internal = 0, stars = 0;
    for (int it = 0; it < 20000; it++) {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        const int B = 1 + (int)(st % 5);
        int nd[5], row0[5], ND = 0, R = 0;
        unsigned long long s2 = st;
        for (int b = 0; b < B; b++) {
            s2 = s2 * 6364136223846793005ull + 1442695040888963407ull;
            nd[b] = (int)((s2 >> 33) % 9) - 1; /* -1 .. 7 */
            row0[b] = R;
            R += nd[b] + 1;
            if (nd[b] > 0) ND += nd[b];
        }
        /* exact-size heap blocks: any read or write past them is reported */
        const size_t n1 = (size_t)(ND ? ND : 1);
        int* drafts = (int*)malloc(n1 * sizeof(int));
        int* parents = (int*)malloc(n1 * sizeof(int));
        int* rows = (int*)malloc(n1 * sizeof(int));
        int* seq = (int*)malloc(n1 * sizeof(int));
        int* nt = (int*)malloc(n1 * sizeof(int));
        int* tg = (int*)malloc(n1 * 7 * sizeof(int));
        int* dst = (int*)malloc(n1 * 7 * sizeof(int));
        int* seen = (int*)calloc(n1, sizeof(int));
        for (int b = 0, o = 0; b < B; o += nd[b] > 0 ? nd[b] : 0, b++)
            for (int j = 0; j < nd[b]; j++) {
                s2 = s2 * 6364136223846793005ull + 1442695040888963407ull;
                drafts[o + j] = 1000 * b + j;
                /* now and then a parent outside [0, j]: clamped, never followed */
                parents[o + j] = (it % 7 == 0 && (s2 >> 60) == 0) ? (int)(s2 >> 40) - 70000 : (int)((s2 >> 33) % (unsigned)(j + 1));
            }
        const int NI = gpt2_tree_dense_tables(drafts, parents, nd, B, row0, rows, seq, tg, nt, dst);
        if (NI < 0 || NI > ND) { printf("NI %d of %d at %d\n", NI, ND, it); return 1; }
        for (int k = 0; k < NI; k++) {
            const int b = seq[k];
            if (b < 0 || b >= B || nt[k] < 1 || nt[k] > 7) { printf("BAD ROW at %d\n", it); return 1; }
            int o = 0;
            for (int q = 0; q < b; q++) o += nd[q] > 0 ? nd[q] : 0;
            const int node = rows[k] - row0[b];
            stars += nt[k] == 7;
            for (int m = 0; m < 7; m++) {
                const int d = dst[k * 7 + m];
                if (m >= nt[k]) { if (d != -1 || tg[k * 7 + m] != -1) { printf("PAD at %d\n", it); return 1; } continue; }
                const int j = d - o;
                if (j < 0 || j >= nd[b] || seen[d]++) { printf("DST at %d\n", it); return 1; }
                int p = parents[d];
                p = p < 0 ? 0 : p > j ? j : p;
                if (p != node || tg[k * 7 + m] != drafts[d]) { printf("CHILD at %d\n", it); return 1; }
                if (m && d <= dst[k * 7 + m - 1]) { printf("ORDER at %d\n", it); return 1; }
            }
        }
        for (int i = 0; i < ND; i++) if (seen[i] != 1) { printf("MISSED draft at %d\n", it); return 1; }
        internal += NI;
        free(drafts); free(parents); free(rows); free(seq); free(nt); free(tg); free(dst); free(seen);
    }
    printf("TREE_TABLES_SAN ok internal=%ld stars=%ld\n", internal, stars);
    return internal > 20000 ? 0 : 2;
}
"""


def test_dense_tables_standalone_under_asan_ubsan(tmp_path):
    """csrc/tree_tables.c (its own translation unit: no device, no allocator)
    and a stand-alone main, both under -fsanitize=address,undefined; the
    program checks 20000 random batches in exact-size heap buffers: every draft
    asked about once, at its (clamped) parent's row, children ascending"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    fn = os.path.join(REPO, "llm.c-paged_amd", "csrc", "tree_tables.c")
    main = tmp_path / "main.c"
    main.write_text(_MAIN)
    exe = tmp_path / "tree_tables_san"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run([cc, *flags, str(fn), str(main), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TREE_TABLES_SAN ok" in r.stdout
