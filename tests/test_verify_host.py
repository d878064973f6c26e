"""Host side of speculative decoding, without a GPU: the pure routing function
gpt2_decode_verify_plan and the n-gram (prompt-lookup) drafter
gpt2_ngram_draft against a numpy restatement; the drafter is also compiled
with a small stand-alone main under -fsanitize=address,undefined and run, and
so are the verify passes' table layout and draft validation
(csrc/verify_tables.c)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pagedattn as pa

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, FP8 = pa.HPA_F32, pa.HPA_BF16, pa.HPA_FP8


# ---------------------------------------------------------------- the plan
def test_plan_fp32_pages_and_rows_take_the_verify_kernel():
    for P in (8, 16, 32, 64):
        for rows in range(1, 9):
            for request in (0, 2):
                assert pa.verify_plan(rows, F32, P, 64, request) == 1, (P, rows, request)


@pytest.mark.parametrize("request_", [0, 1, 2])
def test_plan_refuses_what_the_kernel_does_not_cover(request_):
    for kw in (dict(kv_dtype=BF16), dict(kv_dtype=FP8), dict(max_rows=9), dict(max_rows=0), dict(head_size=128),
               dict(head_size=32), dict(page_size=4), dict(page_size=128)):
        a = dict(max_rows=4, kv_dtype=F32, page_size=16, head_size=64)
        a.update(kw)
        assert pa.verify_plan(request=request_, **a) == 0, (kw, request_)


def test_plan_request_1_is_the_prefill_kernel_and_2_never_exceeds_auto():
    for kv in (F32, BF16, FP8):
        for P in (4, 8, 16, 32, 64, 128):
            for hs in (32, 64, 128):
                for rows in range(0, 11):
                    auto = pa.verify_plan(rows, kv, P, hs, 0)
                    assert pa.verify_plan(rows, kv, P, hs, 1) == 0
                    forced = pa.verify_plan(rows, kv, P, hs, 2)
                    shape_ok = kv == F32 and P in (8, 16, 32, 64) and hs == 64 and 1 <= rows <= 8
                    assert forced == (1 if shape_ok else 0), (rows, kv, P, hs)
                    assert auto <= forced


# ---------------------------------------------------------------- the drafter
def ngram_ref(h, k, max_ngram, min_ngram):
    """the drafter restated: longest n-gram first, most recent earlier
    occurrence with a token after it, up to k following tokens"""
    h = list(h)
    n = len(h)
    if k <= 0 or min_ngram < 1:
        return []
    for g in range(max_ngram, min_ngram - 1, -1):
        for s in range(n - g - 1, -1, -1):
            if h[s:s + g] == h[n - g:]:
                return h[s + g:s + g + k]
    return []


def test_ngram_draft_matches_the_restatement_on_random_histories():
    rng = np.random.default_rng(0)
    hits = 0
    for _ in range(600):
        n = int(rng.integers(0, 40))
        h = rng.integers(0, 4, n)
        k = int(rng.integers(0, 8))
        mx = int(rng.integers(1, 5))
        mn = int(rng.integers(1, mx + 1))
        got = pa.ngram_draft(h, k, mx, mn)
        assert got == ngram_ref(h, k, mx, mn), (h.tolist(), k, mx, mn)
        hits += bool(got)
    assert hits > 200  # the alphabet is small enough that matches are the rule


def test_ngram_draft_named_cases():
    # no match
    assert pa.ngram_draft([1, 2, 3, 4], 3) == []
    # a match at the very start of the history
    assert pa.ngram_draft([7, 8, 9, 1, 2, 7, 8], 2, 2, 2) == [9, 1]
    # a continuation shorter than k: the suffix's only earlier occurrence ends one token before the end
    assert pa.ngram_draft([5, 5], 4, 1, 1) == [5]
    assert pa.ngram_draft([1, 2, 3, 1, 2], 7, 2, 1) == [3, 1, 2]
    # the longest n-gram wins over a more recent shorter match: "1 2" -> 3, though the latest "2" is followed by 9
    assert pa.ngram_draft([1, 2, 3, 0, 2, 9, 1, 2], 1, 2, 1) == [3]
    assert pa.ngram_draft([1, 2, 3, 0, 2, 9, 1, 2], 1, 1, 1) == [9]
    # n < min_ngram, n == min_ngram (no earlier occurrence can exist), k = 0, empty history
    assert pa.ngram_draft([3], 4, 3, 2) == []
    assert pa.ngram_draft([3, 3], 4, 3, 2) == []
    assert pa.ngram_draft([1, 1, 1, 1], 0) == []
    assert pa.ngram_draft([], 4) == []


_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int gpt2_ngram_draft(const int* history, int n, int max_ngram, int min_ngram, int k, int* draft);

/* the restatement, as in the Python test */
static int ref(const int* h, int n, int mx, int mn, int k, int* out) {
    if (k <= 0 || mn < 1) return 0;
    for (int g = mx; g >= mn; g--)
        for (int s = n - g - 1; s >= 0; s--) {
            int eq = 1;
            for (int i = 0; i < g; i++) eq &= h[s + i] == h[n - g + i];
            if (!eq) continue;
            int m = 0;
            for (int i = s + g; i < n && m < k; i++) out[m++] = h[i];
            return m;
        }
    return 0;
}

int main(void) {
    unsigned long long st = 88172645463325252ull;
    long hits = 0;
    for (int it = 0; it < 20000; it++) {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        const int n = (int)(st % 48), k = (int)((st >> 8) % 9), mx = 1 + (int)((st >> 16) % 5);
        const int mn = 1 + (int)((st >> 24) % (unsigned)mx);
        /* exact-size heap blocks: any read or write past them is reported */
        int* h = (int*)malloc((size_t)(n ? n : 1) * sizeof(int));
        int* a = (int*)malloc((size_t)(k ? k : 1) * sizeof(int));
        int* b = (int*)malloc((size_t)(k ? k : 1) * sizeof(int));
        unsigned long long s2 = st;
        for (int i = 0; i < n; i++) { s2 = s2 * 6364136223846793005ull + 1442695040888963407ull; h[i] = (int)((s2 >> 33) % 4); }
        const int ga = gpt2_ngram_draft(h, n, mx, mn, k, a), gb = ref(h, n, mx, mn, k, b);
        if (ga != gb || memcmp(a, b, (size_t)ga * sizeof(int))) { printf("MISMATCH at %d\n", it); return 1; }
        hits += ga > 0;
        free(h); free(a); free(b);
    }
    printf("NGRAM_SAN ok hits=%ld\n", hits);
    return hits > 5000 ? 0 : 2;
}
"""

_SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

# ---------------------------------------------------------------- the verify tables
_VT_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "verify_tables.h"

#define MR VERIFY_MAX_ROWS
#define NAME(type, name) #name,
static const char* names[VT_COUNT] = {VERIFY_TABLES(NAME)};
#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

/* ---- the layout: what the passes write and copy, restated from the kernels' contracts ---- */
static int layout_case(int B, int tree, int sampled) {
    const size_t b = (size_t)B, BD = b * (MR - 1), BR = b * MR, NT = MR - 1;
    const int both = tree && sampled;
    size_t want[VT_COUNT];
    int want_slab[VT_COUNT];
#define W(name, slab, n) (want[VT_##name] = (n), want_slab[VT_##name] = (slab))
    W(drafts, VS_INT, BD);            W(h_drafts, VS_H_INT, tree ? BD : 0);
    W(parents, VS_INT, tree ? BD : 0); W(h_parents, VS_H_INT, tree ? BD : 0);
    W(draft0, VS_INT, b);             W(h_draft0, VS_H_INT, b);
    W(accepted, VS_INT, b);           W(h_accepted, VS_H_INT, b);
    W(path, VS_INT, tree ? BR : 0);   W(h_path, VS_H_INT, tree ? BR : 0);
    W(slot, VS_INT, tree ? BR : 0);
    W(targets, VS_INT, BR);
    W(top, VS_INT, BR);
    W(dense_seq, VS_INT, sampled ? BD : 0);          W(h_dense_seq, VS_H_INT, sampled ? BD : 0);
    W(dense_n, VS_INT, both ? BD : 0);               W(h_dense_n, VS_H_INT, both ? BD : 0);
    W(dense_targets, VS_INT, both ? NT * BD : 0);    W(h_dense_targets, VS_H_INT, both ? NT * BD : 0);
    W(dense_dst, VS_INT, both ? NT * BD : 0);        W(h_dense_dst, VS_H_INT, both ? NT * BD : 0);
    W(h_dense_rows, VS_H_INT, sampled ? BD : 0);
    W(exclude, VS_INT, both ? BD : sampled ? b : 0);
    W(n_exclude, VS_INT, both ? b : 0);
    W(lp, VS_F32, BR);                W(h_lp, VS_H_F32, BR);
    W(w_target, VS_U64, sampled ? BD : 0); W(h_w_target, VS_H_U64, sampled ? BD : 0);
    W(w_total, VS_U64, sampled ? BD : 0);  W(h_w_total, VS_H_U64, sampled ? BD : 0);
    W(anc, VS_U8, tree ? BR : 0);
    W(h_start, VS_H_INT, b); W(h_row0, VS_H_INT, b); W(h_len, VS_H_INT, b);
#undef W
    VerifyLayout L;
    memset(&L, 0xA5, sizeof(L));
    if (verify_tables_layout(B, tree, sampled, &L)) FAIL("layout refused B=%d", B);
    /* every slab at exactly the reported size: a table past its slab is a heap overflow under ASan */
    unsigned char* slab[VS_COUNT];
    for (int s = 0; s < VS_COUNT; s++) {
        const size_t bytes = L.slab_n[s] * verify_slab_elem_bytes(s);
        slab[s] = bytes ? (unsigned char*)malloc(bytes) : NULL;
        if (bytes && !slab[s]) FAIL("malloc");
    }
#define PTR(id) (slab[L.t[id].slab] + L.t[id].off * verify_slab_elem_bytes(L.t[id].slab))
    for (int t = 0; t < VT_COUNT; t++) {
        if (L.t[t].n != want[t]) FAIL("%s: %zu elements, %zu wanted (B=%d tree=%d sampled=%d)", names[t], L.t[t].n, want[t], B, tree, sampled);
        if (!want[t]) continue;
        if (L.t[t].slab != want_slab[t]) FAIL("%s: slab %d, %d wanted", names[t], L.t[t].slab, want_slab[t]);
        if (L.t[t].off + L.t[t].n > L.slab_n[L.t[t].slab]) FAIL("%s leaves its slab", names[t]);
        memset(PTR(t), t + 1, want[t] * verify_slab_elem_bytes(L.t[t].slab)); /* the full extent the kernels write */
    }
    size_t covered[VS_COUNT] = {0};
    for (int t = 0; t < VT_COUNT; t++) {
        if (!want[t]) continue;
        covered[L.t[t].slab] += want[t];
        for (int u = t + 1; u < VT_COUNT; u++)
            if (want[u] && L.t[u].slab == L.t[t].slab && L.t[t].off < L.t[u].off + L.t[u].n && L.t[u].off < L.t[t].off + L.t[t].n)
                FAIL("%s overlaps %s", names[t], names[u]);
        const unsigned char* p = PTR(t); /* nobody wrote over it */
        for (size_t i = 0; i < want[t] * verify_slab_elem_bytes(L.t[t].slab); i++)
            if (p[i] != (unsigned char)(t + 1)) FAIL("%s was overwritten", names[t]);
    }
    for (int s = 0; s < VS_COUNT; s++)
        if (covered[s] != L.slab_n[s]) FAIL("slab %d: %zu elements, its tables hold %zu", s, L.slab_n[s], covered[s]);
    /* tables that move in one copy are neighbours, on the device and in the staging */
#define NEXT(a, c) do { if (L.t[VT_##c].slab != L.t[VT_##a].slab || L.t[VT_##c].off != L.t[VT_##a].off + L.t[VT_##a].n) \
        FAIL(#c " is not right behind " #a " (B=%d tree=%d sampled=%d)", B, tree, sampled); } while (0)
    NEXT(h_start, h_row0); NEXT(h_row0, h_len);
    if (tree) { NEXT(drafts, parents); NEXT(h_drafts, h_parents); NEXT(accepted, path); NEXT(h_accepted, h_path); }
    if (sampled) { NEXT(w_target, w_total); NEXT(h_w_target, h_w_total); }
    if (both) {
        NEXT(dense_seq, dense_n); NEXT(dense_n, dense_targets); NEXT(dense_targets, dense_dst);
        NEXT(h_dense_seq, h_dense_n); NEXT(h_dense_n, h_dense_targets); NEXT(h_dense_targets, h_dense_dst);
    }
    /* every copy of a pass at its largest, on both of its ends (ASan: inside the slabs) */
#define COPY(dev, host, n, es) do { memset(PTR(VT_##dev), 0, (n) * (es)); memset(PTR(VT_##host), 0, (n) * (es)); } while (0)
    memset(PTR(VT_h_start), 0, 3 * b * 4);                    /* -> the dense pass's start, row0, len */
    COPY(draft0, h_draft0, b, 4);
    memset(PTR(VT_drafts), 0, BD * 4);                        /* a chain's drafts, from the caller's array */
    COPY(accepted, h_accepted, b, 4);
    COPY(lp, h_lp, BR, 4);
    if (tree) { COPY(drafts, h_drafts, 2 * BD, 4); COPY(accepted, h_accepted, b + BR, 4); }
    if (sampled) { COPY(dense_seq, h_dense_seq, BD, 4); COPY(w_target, h_w_target, 2 * BD, 8); }
    if (both) COPY(dense_seq, h_dense_seq, (2 + 2 * NT) * BD, 4);
    for (int s = 0; s < VS_COUNT; s++) free(slab[s]);
    return 0;
}

static int layout_main(void) {
    static const int Bs[5] = {1, 2, 3, 64, 65};
    VerifyLayout L;
    if (!verify_tables_layout(0, 0, 0, &L) || !verify_tables_layout(4, 1, 1, NULL)) FAIL("B = 0 or no out accepted");
    for (int i = 0; i < 5; i++)
        for (int k = 0; k < 4; k++)
            if (layout_case(Bs[i], k >> 1, k & 1)) return 1;
    printf("VERIFY_LAYOUT ok\n");
    return 0;
}

/* ---- the validator, restated: each rule on its own, sequence by sequence ---- */
static int ref_check(const int* dr, const int* par, const int* nd, int B, int V, const int* pos, int max_ctx, int* R,
                     int* T, int* ND) {
    *R = *T = *ND = 0;
    for (int b = 0; b < B; b++) {
        if (!(nd[b] >= -1 && nd[b] < MR)) return VERIFY_BAD_N_DRAFT;
        if (pos && pos[b] + nd[b] >= max_ctx) return VERIFY_OVERFLOW;
        *R += nd[b] + 1;
        *ND += nd[b] < 0 ? 0 : nd[b];
        *T = nd[b] + 1 > *T ? nd[b] + 1 : *T;
    }
    if (*ND > 0 && !dr) return VERIFY_NO_DRAFTS;
    for (int i = 0; i < *ND; i++)
        if (!(0 <= dr[i] && dr[i] < V)) return VERIFY_BAD_DRAFT;
    if (!par) return VERIFY_OK;
    int base = 0;
    for (int b = 0; b < B; b++) {
        for (int j = 0; j < nd[b]; j++) {
            if (par[base + j] < 0 || par[base + j] > j) return VERIFY_BAD_PARENT;
            int twins = 0;
            for (int i = 0; i < j; i++) twins += par[base + i] == par[base + j] && dr[base + i] == dr[base + j];
            if (twins) return VERIFY_SAME_SIBLINGS;
        }
        if (nd[b] > 0) base += nd[b];
    }
    return VERIFY_OK;
}

static int one(const int* dr, const int* par, int nd, int V) { /* one sequence, no context check */
    VerifyDrafts e;
    return verify_drafts_check(dr, par, &nd, 1, V, NULL, 0, &e);
}

static int check_main(void) {
    const int V = 50;
    VerifyDrafts e;
    int chain[8] = {0, 1, 2, 3, 4, 5, 6, 7}, self[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    /* n_draft = -2, -1, 0, 7, 8 */
    if (one(chain, NULL, -2, V) != VERIFY_BAD_N_DRAFT || one(chain, NULL, 8, V) != VERIFY_BAD_N_DRAFT) FAIL("n_draft -2 / 8");
    if (one(chain, NULL, -1, V) || one(NULL, NULL, 0, V) || one(chain, NULL, 7, V) || one(chain, self, 7, V)) FAIL("n_draft -1 / 0 / 7");
    int nd3[3] = {-1, 0, 7};
    if (verify_drafts_check(chain, NULL, nd3, 3, V, NULL, 0, &e) || e.R != 9 || e.T != 8 || e.ND != 7) FAIL("R, T, ND");
    nd3[0] = nd3[2] = -1; nd3[1] = -1;
    if (verify_drafts_check(NULL, NULL, nd3, 3, V, NULL, 0, &e) || e.R != 0 || e.T != 0 || e.ND != 0) FAIL("nobody takes part");
    if (one(NULL, NULL, 1, V) != VERIFY_NO_DRAFTS) FAIL("no drafts");
    /* the context: pos + n_draft + 1 <= max_ctx */
    int pos1 = 92, n7 = 7;
    if (verify_drafts_check(chain, NULL, &n7, 1, V, &pos1, 100, &e) != VERIFY_OK) FAIL("fits exactly");
    if (verify_drafts_check(chain, NULL, &n7, 1, V, &pos1, 99, &e) != VERIFY_OVERFLOW || e.seq != 0 || e.value != 7) FAIL("overflow");
    /* a draft id of -1, of V, of V - 1 */
    int ids[3] = {4, -1, 5};
    if (verify_drafts_check(ids, NULL, &(int){3}, 1, V, NULL, 0, &e) != VERIFY_BAD_DRAFT || e.i != 1 || e.value != -1) FAIL("id -1");
    ids[1] = V;
    if (one(ids, NULL, 3, V) != VERIFY_BAD_DRAFT) FAIL("id V");
    ids[1] = V - 1;
    if (one(ids, NULL, 3, V)) FAIL("id V - 1");
    /* a parent of -1, j, j + 1 (draft j = 2) */
    int par[3] = {0, 0, -1};
    if (verify_drafts_check(ids, par, &(int){3}, 1, V, NULL, 0, &e) != VERIFY_BAD_PARENT || e.j != 2 || e.value != -1) FAIL("parent -1");
    par[2] = 2;
    if (one(ids, par, 3, V)) FAIL("parent j");
    par[2] = 3;
    if (one(ids, par, 3, V) != VERIFY_BAD_PARENT) FAIL("parent j + 1");
    /* two siblings with one token; the same token under different parents */
    int tw[3] = {9, 7, 9}, tp[3] = {0, 0, 0};
    if (verify_drafts_check(tw, tp, &(int){3}, 1, V, NULL, 0, &e) != VERIFY_SAME_SIBLINGS || e.i != 0 || e.j != 2) FAIL("twins");
    tp[2] = 1;
    if (one(tw, tp, 3, V)) FAIL("one token under two parents");
    if (one(tw, NULL, 3, V)) FAIL("a chain may repeat a token");

    /* seeded random trees, mostly valid, each rule broken now and then */
    unsigned long long st = 88172645463325252ull;
    long seen[VERIFY_SAME_SIBLINGS + 1] = {0};
#define RND(n) (st ^= st << 13, st ^= st >> 7, st ^= st << 17, (int)((st >> 11) % (unsigned)(n)))
    for (int it = 0; it < 20000; it++) {
        const int B = 1 + RND(4), Vr = 3 + RND(6), max_ctx = 64, tree = RND(4) != 0;
        int nd[4], pos[4], total = 0;
        for (int b = 0; b < B; b++) {
            nd[b] = RND(60) == 0 ? (RND(2) ? -2 : MR) : RND(MR + 1) - 1;
            pos[b] = RND(40) == 0 ? max_ctx - RND(MR + 1) : RND(40);
            if (nd[b] > 0) total += nd[b];
        }
        /* exact-size heap blocks: any read past them is reported */
        int* dr = (int*)malloc((size_t)(total ? total : 1) * sizeof(int));
        int* pa = (int*)malloc((size_t)(total ? total : 1) * sizeof(int));
        for (int b = 0, k = 0; b < B; b++)
            for (int j = 0; j < nd[b]; j++, k++) {
                dr[k] = RND(150) == 0 ? (RND(2) ? -1 : Vr) : RND(Vr);
                pa[k] = RND(150) == 0 ? (RND(2) ? -1 : j + 1) : RND(j + 1);
            }
        int R, T, ND;
        const int want = ref_check(dr, tree ? pa : NULL, nd, B, Vr, pos, max_ctx, &R, &T, &ND);
        const int got = verify_drafts_check(dr, tree ? pa : NULL, nd, B, Vr, pos, max_ctx, &e);
        if (got != want || (!got && (e.R != R || e.T != T || e.ND != ND))) FAIL("MISMATCH at %d: %d, %d wanted", it, got, want);
        seen[got]++;
        free(dr); free(pa);
    }
    for (int c = 0; c <= VERIFY_SAME_SIBLINGS; c++)
        if (c != VERIFY_NO_DRAFTS && seen[c] < 50) FAIL("code %d met only %ld times", c, seen[c]);
    printf("VERIFY_CHECK ok valid=%ld\n", seen[VERIFY_OK]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "layout")) return layout_main();
    if (argc == 2 && !strcmp(argv[1], "check")) return check_main();
    return 2;
}
"""


@pytest.fixture(scope="module")
def verify_tables_san(tmp_path_factory):
    """csrc/verify_tables.c (no device, no allocator) and a stand-alone main,
    both under -fsanitize=address,undefined, built once"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    csrc = os.path.join(REPO, "llm.c-paged_amd", "csrc")
    d = tmp_path_factory.mktemp("verify_tables")
    main = d / "main.c"
    main.write_text(_VT_MAIN)
    exe = d / "verify_tables_san"
    subprocess.run([cc, "-std=gnu11", "-Wall", "-Wextra", "-Werror", *_SAN_FLAGS, "-I", csrc,
                    os.path.join(csrc, "verify_tables.c"), str(main), "-o", str(exe)], check=True)
    return str(exe)


def test_verify_tables_layout_under_asan_ubsan(verify_tables_san):
    """B in {1, 2, 3, 64, 65} x (tree, sampled): every slab allocated at exactly
    the reported size, every table written over the extent the kernels write
    and the largest copy of every pass made on both ends; the tables of a slab
    are disjoint, fill it, and the ones that move in one copy are neighbours"""
    r = subprocess.run([verify_tables_san, "layout"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "VERIFY_LAYOUT ok" in r.stdout


def test_verify_drafts_check_under_asan_ubsan(verify_tables_san):
    """the named refusals (n_draft -2 / 8, ids -1 / V, parents -1 / j + 1, twin
    siblings, overflow) and acceptances, then 20000 seeded random batches of
    trees and chains against a restatement"""
    r = subprocess.run([verify_tables_san, "check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "VERIFY_CHECK ok" in r.stdout


def test_ngram_draft_standalone_under_asan_ubsan(tmp_path):
    """csrc/ngram_draft.c (the drafter's own translation unit: no device, no
    allocator) and a stand-alone main, both under -fsanitize=address,undefined;
    the program compares 20000 random histories in exact-size heap buffers
    against the restatement"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    fn = os.path.join(REPO, "llm.c-paged_amd", "csrc", "ngram_draft.c")
    main = tmp_path / "main.c"
    main.write_text(_MAIN)
    exe = tmp_path / "ngram_san"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run([cc, *flags, str(fn), str(main), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "NGRAM_SAN ok" in r.stdout
