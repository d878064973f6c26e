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

/* The tree drafter (gpt2_ngram_draft_tree, paged_infer.h): the same scan, every
 * occurrence's continuation inserted into a trie over (draft, parents).  Node 0
 * is the root (the pending token); draft j is node j + 1. */
#define NGRAM_TREE_MAX_NODES 7 /* HPA_VERIFY_MAX_ROWS - 1 */

int gpt2_ngram_draft_tree(const int* history, int n, int max_ngram, int min_ngram, int max_nodes, int depth,
                          int max_branches, int* draft, int* parents);

int gpt2_ngram_draft_tree(const int* history, int n, int max_ngram, int min_ngram, int max_nodes, int depth,
                          int max_branches, int* draft, int* parents) {
    if (!history || !draft || !parents || min_ngram < 1 || depth < 1 || max_branches < 1) return 0;
    if (max_nodes < 1 || max_nodes > NGRAM_TREE_MAX_NODES) return 0;
    int nodes = 0, branches = 0;
    for (int g = max_ngram; g >= min_ngram; g--) {
        for (int s = n - g - 1; s >= 0; s--) {
            if (memcmp(history + s, history + n - g, (size_t)g * sizeof(int))) continue;
            int m = n - (s + g);
            if (m > depth) m = depth;
            int cur = 0, added = 0;
            for (int i = 0; i < m; i++) {
                const int t = history[s + g + i];
                int c = 0; /* the child of cur that carries t, as a node index (0: none) */
                for (int j = 0; j < nodes && !c; j++)
                    if (parents[j] == cur && draft[j] == t) c = j + 1;
                if (!c) {
                    if (nodes == max_nodes) break;
                    draft[nodes] = t;
                    parents[nodes] = cur;
                    c = ++nodes;
                    added = 1;
                }
                cur = c;
            }
            branches += added;
            if (nodes == max_nodes || branches == max_branches) return nodes;
        }
    }
    return nodes;
}
