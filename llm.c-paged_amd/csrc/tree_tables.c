/* tree_tables.c -- the dense-route tables of sampled tree speculation
 * (gpt2_tree_dense_tables, paged_infer.h): which rows of a tree pass go
 * through the LOGITS GEMM, and which ids each of them is asked about.  Host
 * arithmetic on the caller's arrays only: no device, no allocation, no I/O, so
 * it builds and runs on its own (tests/test_tree_spec_ref64.py compiles it
 * under ASan + UBSan). */
#define TREE_MAX_DRAFTS 7 /* HPA_VERIFY_MAX_ROWS - 1 */

int gpt2_tree_dense_tables(const int* drafts, const int* parents, const int* n_draft, int B, const int* row0, int* rows,
                           int* seq, int* targets, int* n_targets, int* dst);

int gpt2_tree_dense_tables(const int* drafts, const int* parents, const int* n_draft, int B, const int* row0, int* rows,
                           int* seq, int* targets, int* n_targets, int* dst) {
    if (!n_draft || !row0 || !rows || !seq || !targets || !n_targets || !dst || B <= 0) return 0;
    int ni = 0, nd = 0;
    for (int b = 0; b < B; b++) {
        int n = n_draft[b] > TREE_MAX_DRAFTS ? TREE_MAX_DRAFTS : n_draft[b];
        if (n <= 0) continue;
        if (!drafts || !parents) return ni;
        /* node i is internal iff some draft hangs from it; a leaf never reaches the GEMM */
        for (int i = 0; i < n; i++) { /* node n (the last draft) cannot be a parent */
            int m = 0;
            for (int j = i; j < n; j++) { /* draft j's parent lies in [0, j]: clamped like the device tables */
                int p = parents[nd + j];
                p = p < 0 ? 0 : p > j ? j : p;
                if (p != i) continue;
                if (m == 0) {
                    rows[ni] = row0[b] + i;
                    seq[ni] = b;
                }
                targets[ni * TREE_MAX_DRAFTS + m] = drafts[nd + j];
                dst[ni * TREE_MAX_DRAFTS + m] = nd + j;
                m++;
            }
            if (m == 0) continue;
            for (int k = m; k < TREE_MAX_DRAFTS; k++) {
                targets[ni * TREE_MAX_DRAFTS + k] = -1;
                dst[ni * TREE_MAX_DRAFTS + k] = -1;
            }
            n_targets[ni++] = m;
        }
        nd += n_draft[b]; /* the packing of `drafts`: every draft counts */
    }
    return ni;
}
