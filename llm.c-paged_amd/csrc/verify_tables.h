/* verify_tables.h -- internal: the workspace layout and the draft validation
 * of the speculative verify passes (verify_tables.c; used by paged_infer.c
 * and by tests/test_verify_host.py's stand-alone program).  Not public API. */
#ifndef VERIFY_TABLES_H
#define VERIFY_TABLES_H
#include <stddef.h>

#define VERIFY_MAX_ROWS 8 /* HPA_VERIFY_MAX_ROWS (hip_paged_attn.h) */

/* Every table of a verify pass, X(element type, name), device tables first.
 * B sequences, MR = VERIFY_MAX_ROWS rows each at most, BD = B * (MR - 1)
 * drafts at most; extents and order: verify_tables_layout. */
#define VERIFY_TABLES(X)                                                                             \
    X(int, drafts)             /* [BD] packed draft ids */                                           \
    X(int, parents)            /* [BD] tree: draft j's parent node */                                \
    X(int, draft0)             /* [B] a sequence's first packed draft */                             \
    X(int, accepted)           /* [B] drafts accepted */                                             \
    X(int, path)               /* [B * MR] tree: the accepted nodes */                               \
    X(int, slot)               /* [B * MR] tree: the rows' K/V append slots */                       \
    X(int, targets)            /* [B * MR] greedy: the rows' SCORE targets */                        \
    X(int, top)                /* [B * MR] greedy: the rows' greedy ids */                           \
    X(int, dense_seq)          /* [BD] sampled: the dense route's rows' sequences */                 \
    X(int, dense_n)            /* [BD] sampled tree: ids asked of each internal node */              \
    X(int, dense_targets)      /* [BD * (MR - 1)] sampled tree: those ids */                         \
    X(int, dense_dst)          /* [BD * (MR - 1)] sampled tree: the packed draft each id is */       \
    X(int, exclude)            /* sampled: the rejected id [B]; with a tree the lists [BD] */        \
    X(int, n_exclude)          /* [B] sampled tree: the lists' lengths */                            \
    X(float, lp)               /* [B * MR] greedy: the rows' log-probabilities */                    \
    X(unsigned long long, w_target) /* [BD] sampled: a draft's mass */                               \
    X(unsigned long long, w_total)  /* [BD] sampled: its row's total mass */                         \
    X(unsigned char, anc)      /* [B * MR] tree: the rows' ancestor masks */                         \
    X(int, h_start)            /* host staging from here on: [B] the pass's start positions, */     \
    X(int, h_row0)             /* [B] first packed rows */                                           \
    X(int, h_len)              /* [B] and row counts */                                              \
    X(int, h_draft0)           /* [B] */                                                             \
    X(int, h_drafts)           /* [BD] tree */                                                       \
    X(int, h_parents)          /* [BD] tree */                                                       \
    X(int, h_accepted)         /* [B] */                                                             \
    X(int, h_path)             /* [B * MR] tree */                                                   \
    X(int, h_dense_rows)       /* [BD] sampled: the dense route's packed rows (host only) */         \
    X(int, h_dense_seq)        /* [BD] sampled */                                                    \
    X(int, h_dense_n)          /* [BD] sampled tree */                                               \
    X(int, h_dense_targets)    /* [BD * (MR - 1)] sampled tree */                                    \
    X(int, h_dense_dst)        /* [BD * (MR - 1)] sampled tree */                                    \
    X(float, h_lp)             /* [B * MR] */                                                        \
    X(unsigned long long, h_w_target) /* [BD] sampled */                                             \
    X(unsigned long long, h_w_total)  /* [BD] sampled */

#define VERIFY_TABLE_ID(type, name) VT_##name,
enum { VERIFY_TABLES(VERIFY_TABLE_ID) VT_COUNT };

/* the slabs, one allocation each: device by element type, then host */
enum { VS_INT, VS_F32, VS_U64, VS_U8, VS_H_INT, VS_H_F32, VS_H_U64, VS_COUNT };
#define VS_HOST VS_H_INT /* slabs from here on are host memory */

typedef struct {
    int slab;      /* VS_* */
    size_t off, n; /* in elements of the slab; n = 0: not part of this layout */
} VerifyTable;

typedef struct {
    size_t slab_n[VS_COUNT]; /* elements */
    VerifyTable t[VT_COUNT];
} VerifyLayout;

size_t verify_slab_elem_bytes(int slab);

/* the layout for B sequences that serves the chain passes and, with tree /
 * sampled, those passes too; nonzero: B < 1 or no out */
int verify_tables_layout(int B, int tree, int sampled, VerifyLayout* out);

/* what verify_drafts_check refuses, in the order it looks */
enum {
    VERIFY_OK = 0,
    VERIFY_BAD_N_DRAFT, /* n_draft[seq] = value is outside [-1, MR - 1] */
    VERIFY_OVERFLOW,    /* value = n_draft[seq] drafts and the pending id pass max_ctx */
    VERIFY_NO_DRAFTS,   /* ND > 0 and drafts is NULL */
    VERIFY_BAD_DRAFT,   /* packed draft i = value is outside [0, V) */
    VERIFY_BAD_PARENT,  /* parent value of draft j of seq is outside [0, j] */
    VERIFY_SAME_SIBLINGS /* drafts i < j of seq: one parent, one token */
};

typedef struct {
    int R, T, ND;          /* rows of the pass, most rows of a sequence, drafts (valid on VERIFY_OK) */
    int seq, i, j, value;  /* what was refused (see the codes) */
} VerifyDrafts;

/* n_draft [B] in [-1, MR - 1] (-1: the sequence sits out); drafts / parents
 * packed in sequence order (parents NULL: chains); pos [B] (nullable: no
 * context check) the sequences' positions */
int verify_drafts_check(const int* drafts, const int* parents, const int* n_draft, int B, int V, const int* pos,
                        int max_ctx, VerifyDrafts* out);

#endif
