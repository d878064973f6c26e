/* ngram_draft.c -- the n-gram (prompt-lookup) drafter of speculative decoding
 * (gpt2_ngram_draft, paged_infer.h).  Host arithmetic on the caller's arrays
 * only: no device, no allocation, no I/O, so it builds and runs on its own
 * (tests/test_verify_host.py compiles it under ASan + UBSan). */
#include <string.h>

int gpt2_ngram_draft(const int* history, int n, int max_ngram, int min_ngram, int k, int* draft);

int gpt2_ngram_draft(const int* history, int n, int max_ngram, int min_ngram, int k, int* draft) {
    if (!history || !draft || k <= 0 || min_ngram < 1) return 0;
    for (int g = max_ngram; g >= min_ngram; g--) {
        /* an earlier occurrence [s, s + g) of the last g tokens with a token after it: s + g <= n - 1 */
        for (int s = n - g - 1; s >= 0; s--) {
            if (memcmp(history + s, history + n - g, (size_t)g * sizeof(int))) continue;
            int m = n - (s + g);
            if (m > k) m = k;
            memcpy(draft, history + s + g, (size_t)m * sizeof(int));
            return m;
        }
    }
    return 0;
}
