"""Host side of speculative decoding, without a GPU: the pure routing function
gpt2_decode_verify_plan and the n-gram (prompt-lookup) drafter
gpt2_ngram_draft against a numpy restatement; the drafter is also compiled
with a small stand-alone main under -fsanitize=address,undefined and run."""
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
