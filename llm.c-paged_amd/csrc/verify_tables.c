/* verify_tables.c -- the workspace layout of the speculative verify passes
 * (gpt2_decode_verify, _sampled, _tree, _tree_sampled: paged_infer.c) and the
 * arithmetic part of their draft validation.  Host arithmetic only: no device,
 * no allocation, no I/O, so it builds and runs on its own
 * (tests/test_verify_host.py compiles it under ASan + UBSan).
 *
 * The passes move several tables in one copy; those tables must stay
 * neighbours, in this order, on the device and in the host staging alike:
 *   - drafts, parents (tree): parents == drafts + BD; one upload of BD + ND ints
 *   - accepted, path (tree): path == accepted + B; one download of B + B * MR ints
 *   - w_target, w_total: w_total == w_target + BD; one download of 2 * BD words
 *   - dense_seq, dense_n, dense_targets, dense_dst (sampled tree): one upload
 *     of (2 + 2 * (MR - 1)) * BD ints
 *   - h_start, h_row0, h_len: one upload of 3 * B ints into the dense pass's
 *     row tables
 * The order of the PUT lines below is that order. */
#include "verify_tables.h"

#define MR VERIFY_MAX_ROWS

size_t verify_slab_elem_bytes(int slab) {
    switch (slab) {
        case VS_U8: return 1;
        case VS_U64: case VS_H_U64: return sizeof(unsigned long long);
        case VS_F32: case VS_H_F32: return sizeof(float);
        default: return sizeof(int);
    }
}

int verify_tables_layout(int B, int tree, int sampled, VerifyLayout* out) {
    if (B < 1 || !out) return 1;
    const size_t b = (size_t)B, BD = b * (MR - 1), BR = b * MR, NT = MR - 1;
    const int both = tree && sampled;
    for (int s = 0; s < VS_COUNT; s++) out->slab_n[s] = 0;
    for (int t = 0; t < VT_COUNT; t++) out->t[t] = (VerifyTable){0, 0, 0};
#define PUT(name, s, count) \
    (out->t[VT_##name] = (VerifyTable){s, out->slab_n[s], count}, out->slab_n[s] += (count))
    PUT(drafts, VS_INT, BD);
    if (tree) PUT(parents, VS_INT, BD);
    PUT(draft0, VS_INT, b);
    PUT(accepted, VS_INT, b);
    if (tree) PUT(path, VS_INT, BR);
    if (tree) PUT(slot, VS_INT, BR);
    PUT(targets, VS_INT, BR);
    PUT(top, VS_INT, BR);
    if (sampled) PUT(dense_seq, VS_INT, BD);
    if (both) PUT(dense_n, VS_INT, BD);
    if (both) PUT(dense_targets, VS_INT, NT * BD);
    if (both) PUT(dense_dst, VS_INT, NT * BD);
    if (sampled) PUT(exclude, VS_INT, both ? BD : b);
    if (both) PUT(n_exclude, VS_INT, b);
    PUT(lp, VS_F32, BR);
    if (sampled) PUT(w_target, VS_U64, BD);
    if (sampled) PUT(w_total, VS_U64, BD);
    if (tree) PUT(anc, VS_U8, BR);

    PUT(h_start, VS_H_INT, b);
    PUT(h_row0, VS_H_INT, b);
    PUT(h_len, VS_H_INT, b);
    PUT(h_draft0, VS_H_INT, b);
    if (tree) PUT(h_drafts, VS_H_INT, BD);
    if (tree) PUT(h_parents, VS_H_INT, BD);
    PUT(h_accepted, VS_H_INT, b);
    if (tree) PUT(h_path, VS_H_INT, BR);
    if (sampled) PUT(h_dense_rows, VS_H_INT, BD);
    if (sampled) PUT(h_dense_seq, VS_H_INT, BD);
    if (both) PUT(h_dense_n, VS_H_INT, BD);
    if (both) PUT(h_dense_targets, VS_H_INT, NT * BD);
    if (both) PUT(h_dense_dst, VS_H_INT, NT * BD);
    PUT(h_lp, VS_H_F32, BR);
    if (sampled) PUT(h_w_target, VS_H_U64, BD);
    if (sampled) PUT(h_w_total, VS_H_U64, BD);
#undef PUT
    return 0;
}

int verify_drafts_check(const int* drafts, const int* parents, const int* n_draft, int B, int V, const int* pos,
                        int max_ctx, VerifyDrafts* out) {
    *out = (VerifyDrafts){0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < B; b++) {
        out->seq = b;
        out->value = n_draft[b];
        if (n_draft[b] < -1 || n_draft[b] > MR - 1) return VERIFY_BAD_N_DRAFT;
        if (pos && pos[b] + n_draft[b] + 1 > max_ctx) return VERIFY_OVERFLOW;
        out->R += n_draft[b] + 1;
        if (n_draft[b] > 0) out->ND += n_draft[b];
        if (n_draft[b] + 1 > out->T) out->T = n_draft[b] + 1;
    }
    if (out->ND && !drafts) return VERIFY_NO_DRAFTS;
    for (int i = 0; i < out->ND; i++)
        if (drafts[i] < 0 || drafts[i] >= V) {
            out->i = i;
            out->value = drafts[i];
            return VERIFY_BAD_DRAFT;
        }
    if (!parents) return VERIFY_OK;
    /* draft j of a sequence is node j + 1: its parent a node in [0, j], no sibling with its token */
    for (int b = 0, nd = 0; b < B; nd += n_draft[b] > 0 ? n_draft[b] : 0, b++)
        for (int j = 0; j < n_draft[b]; j++) {
            const int pj = parents[nd + j];
            out->seq = b;
            out->j = j;
            out->value = pj;
            if (pj < 0 || pj > j) return VERIFY_BAD_PARENT;
            for (int i = 0; i < j; i++)
                if (parents[nd + i] == pj && drafts[nd + i] == drafts[nd + j]) {
                    out->i = i;
                    return VERIFY_SAME_SIBLINGS;
                }
        }
    return VERIFY_OK;
}
