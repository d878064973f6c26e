/*
 * paged_infer.h -- drop-in for the API of mx60s/llm.c-paged paged_infer.c
 * (GPT-2 inference over a paged KV cache), backed by MI355X kernels.
 *
 * Reference-named functions keep the reference signatures
 * (paged_infer.c:24-302, :436-745, :826-951).  Their data may live on the
 * host or in device memory: host buffers are staged through HBM and the
 * result copied back, so a caller written for the reference works unchanged.
 * The layer functions compute on the GPU with the reference's arithmetic
 * order (hpa_ref_* kernels).
 *
 * The decode hot path is additive: gpt2_decode_* run one batched decode
 * step (one token for each of B sequences at absolute positions) entirely
 * on device through hand-written gfx950 kernels, the page pool in HBM and
 * per-sequence block tables from the BlockManager.  gpt2_forward() is
 * implemented on top of it with corrected semantics (all L layers, absolute
 * positions, one page list per sequence).
 */
#ifndef PAGED_INFER_H
#define PAGED_INFER_H
#include <stddef.h>
#include <stdint.h>

#include "block_manager.h"
#ifdef __cplusplus
extern "C" {
#endif

/* paged_infer.c:397-403 */
typedef struct {
    int max_seq_len;
    int vocab_size;
    int num_layers;
    int num_heads;
    int channels;
} GPT2Config;

/* paged_infer.c:308-326; DEVICE pointers into params_memory */
#define NUM_PARAMETER_TENSORS 16
typedef struct {
    float* wte;      /* (V, C) */
    float* wpe;      /* (maxT, C) */
    float* ln1w;     /* (L, C) */
    float* ln1b;     /* (L, C) */
    float* qkvw;     /* (L, 3C, C) */
    float* qkvb;     /* (L, 3C) */
    float* attprojw; /* (L, C, C) */
    float* attprojb; /* (L, C) */
    float* ln2w;     /* (L, C) */
    float* ln2b;     /* (L, C) */
    float* fcw;      /* (L, 4C, C) */
    float* fcb;      /* (L, 4C) */
    float* fcprojw;  /* (L, C, 4C) */
    float* fcprojb;  /* (L, C) */
    float* lnfw;     /* (C) */
    float* lnfb;     /* (C) */
} ParameterTensors;

/* the caller-visible outputs of gpt2_forward (paged_infer.c:350-375 keeps 23
 * activation tensors; decode needs only these, host-readable) */
typedef struct {
    float* logits; /* (B, T, V): row T-1 of every b written by gpt2_forward */
    float* probs;  /* (B, T, V): softmax of those rows */
} ActivationTensors;

typedef struct GPT2Decode GPT2Decode;

/* paged_infer.c:405-434 (training-only fields dropped) */
typedef struct {
    GPT2Config config;
    ParameterTensors params;
    size_t param_sizes[NUM_PARAMETER_TENSORS];
    float* params_memory; /* device */
    size_t num_parameters;
    ActivationTensors acts;
    float* acts_memory;   /* managed memory behind acts */
    int batch_size;
    int seq_len;
    int* inputs;
    int* targets;
    float mean_loss;
    BlockManager* manager; /* kv cache stuff (set by the caller, paged_infer.c:986-987) */
    GPT2Decode* decode;    /* device decode engine (lazily created) */
} GPT2;

/* ---------------- reference API ---------------- */
void encoder_forward(float* out, int* inp, float* wte, float* wpe, int B, int T, int C);
void layernorm_forward(float* out, float* mean, float* rstd, float* inp, float* weight, float* bias,
                       int B, int T, int C);
void matmul_forward(float* out, float* inp, float* weight, float* bias, int B, int T, int C, int OC);
void matmul_cached(float* out, float* inp, float* weight, float* bias, int B, int T, int C, int OC);
void attention_paged(float* out, float* preatt, float* att, float* inp, float** key_blocks,
                     float** value_blocks, int B, int T, int C, int NH, int offset);
void gelu_forward(float* out, float* inp, int N);
void residual_forward(float* out, float* inp1, float* inp2, int N);
void softmax_forward(float* probs, float* logits, int B, int T, int V);
void add_to_cache(BlockManager* manager, float* qkv, int B, int T, int C,
                  int how_many_tokens_to_copy_from_the_end_of_sequence);
void gpt2_build_from_checkpoint(GPT2* model, const char* checkpoint_path);
void gpt2_forward(GPT2* model, int* inputs, int* targets, size_t B, size_t T, size_t max_total,
                  int offset);
void gpt2_free(GPT2* model);
unsigned int random_u32(unsigned long long* state);
float random_f32(unsigned long long* state);
int sample_mult(float* probabilities, int n, float coin);
int* generate_tokens_from_logits(float* probs, int B, int T, int V);
void print_generated_sequence(int* tokens, int B, int T);   /* :930-935 */

/* tokenizer, decode only (paged_infer.c:852-928); file written by
 * train_gpt2.py:350-363 */
typedef struct {
    uint32_t vocab_size;
    char** token_table;
    int init_ok;
} Tokenizer;
void safe_printf(const char* piece);
void tokenizer_init(Tokenizer* tokenizer, const char* filename);
const char* tokenizer_decode(Tokenizer* tokenizer, uint32_t token_id);
void tokenizer_free(Tokenizer* tokenizer);

/* attention_paged with the page size as an argument (the reference fixes
 * BLOCK_SIZE = 32); attention_paged() uses BLOCK_SIZE */
void attention_paged_bs(float* out, float* preatt, float* att, float* inp, float** key_blocks,
                        float** value_blocks, int B, int T, int C, int NH, int offset,
                        int block_size);

/* ---------------- model construction (additive) ---------------- */
/* upload host params (checkpoint order) to the device; 0 on success */
int gpt2_build_from_params(GPT2* model, GPT2Config config, const float* host_params);
/* seeded synthetic GPT-2 weights (the reference xorshift, paged_infer.c:826-835) */
int gpt2_build_synthetic(GPT2* model, GPT2Config config, unsigned long long seed);
size_t gpt2_num_parameters(GPT2Config config);
int gpt2_synthetic_params(GPT2Config config, unsigned long long seed, float* host_params);
int gpt2_write_checkpoint(const char* path, GPT2Config config, const float* host_params);
/* version 1 (fp32) or 2 (bf16 weights, LN fp32 and last: train_gpt2.py:267-293,
 * rounded to nearest even as torch .to(bfloat16)) */
int gpt2_write_checkpoint_ex(const char* path, GPT2Config config, const float* host_params, int version);
/* host-only reader of v1 and v2 checkpoints: config (nullable) from the
 * header; host_params (nullable: header only) receives the parameters in
 * ParameterTensors order as fp32 (bf16 widened exactly).  Nonzero + stderr
 * on a bad file (gpt2_build_from_checkpoint prints and exits instead, as
 * the reference :436-502). */
int gpt2_read_checkpoint(const char* path, GPT2Config* config, float* host_params);

/* heap handle for FFI callers (ctypes / cgo) that cannot size GPT2 */
GPT2* gpt2_alloc(void);
void gpt2_release(GPT2* model); /* gpt2_free + free */
void gpt2_set_manager(GPT2* model, BlockManager* manager);
float* gpt2_acts_logits(GPT2* model);
float* gpt2_acts_probs(GPT2* model);

/* ---------------- decode engine (the MI355X hot path) ---------------- */
/* B sequences, page_size tokens per page, up to max_ctx tokens per sequence.
 * Uses model->manager when it was set by the caller (its block_size becomes
 * the page size), otherwise creates one sized B x ceil(max_ctx/page_size). */
int  gpt2_decode_init(GPT2* model, int B, int page_size, int max_ctx);
/* the same with the KV pool's storage type: HPA_F32 (0, default), HPA_BF16
 * (1: BASELINE config 5; page size a multiple of 8) or HPA_FP8 (2: OCP e4m3fn
 * codes with one fp32 scale per (layer, K|V, head), hip_paged_attn.h; page
 * size 16, 32 or 64, else the call fails with a message).  fp8 storage is
 * lossy (3 mantissa bits) and halves the bf16 pool's bytes again; the scales
 * start at 1.0 (gpt2_decode_set_kv_scales).  With an fp8 pool the layer loop
 * runs chain form 6 where it applies (auto and form 5: C = 768, 12 heads,
 * B <= 64, fp32 weights) and five launches per layer for every other pick
 * (bf16 weights included: gpt2_decode_layer_kernel() then reports 0). */
int  gpt2_decode_init_ex(GPT2* model, int B, int page_size, int max_ctx, int kv_dtype);
/* ... and the weights' storage type: HPA_F32 (0, default) or HPA_BF16 (1:
 * "bf16 decode" -- the layer and logits weights packed bf16 in HBM, GEMM
 * inputs rounded to bf16 after their LayerNorm, fp32 accumulation on
 * v_mfma_f32_16x16x32_bf16; LayerNorm, attention, residuals, GELU, softmax
 * stay fp32) */
int  gpt2_decode_init_w(GPT2* model, int B, int page_size, int max_ctx, int kv_dtype, int w_dtype);
/* one decode step for every sequence: tokens[b] (host) at position pos[b];
 * tokens == NULL feeds back the previous step's greedy ids (device-resident).
 * next_tokens (host, may be NULL) receives argmax(logits[b]). */
int  gpt2_decode_step(GPT2* model, const int* tokens, int* next_tokens);
/* prefill: tokens[b*T + t] (host) at positions pos[b] + t for every sequence,
 * all T tokens in one pass (B*T-row GEMMs, causal multi-query paged
 * attention on MFMA); afterwards logits / next ids are those of each
 * sequence's last token and pos[b] += T, so decode continues with
 * gpt2_decode_step(model, NULL, ...). */
int  gpt2_decode_prefill(GPT2* model, const int* tokens, int T, int* next_tokens);
/* continuous batching: one pass over lens[b] >= 0 new tokens per sequence
 * (tokens packed in sequence order, sum(lens) of them): prompts of newly
 * admitted sequences and single decode tokens of running ones go through
 * the same call.  Sequences with lens[b] = 0 are untouched (position, next
 * id, sampler state).  next_tokens[b] is each sequence's next id. */
int  gpt2_decode_prefill_ragged(GPT2* model, const int* tokens, const int* lens, int* next_tokens);
/* prompt scoring: everything gpt2_decode_prefill_ragged does (K/V appended,
 * positions advanced, the last row's logits and pick, lens[b] = 0 sequences
 * untouched) and, for every packed row r (host arrays of sum(lens) entries,
 * packed like tokens):
 *   logprobs[r] = log softmax(logits_r)[targets[r]], 0 where targets[r] == -1
 *   top_ids[r]  = row r's greedy id (lowest index on ties); nullable
 * The logits of the rows never reach memory: the rows go through a SCORE GEMM
 * (HPA_FEPI_SCORE, a log-softmax epilogue) in chunks of
 * gpt2_decode_set_score_chunk rows, whose partial workspace (allocated on
 * first use, freed with the engine) is the only buffer that grows with the
 * vocabulary.  A target outside [-1, vocab_size) returns nonzero with a
 * message and changes nothing. */
int  gpt2_decode_score(GPT2* model, const int* tokens, const int* lens, const int* targets, float* logprobs,
                       int* top_ids, int* next_tokens);
/* rows per SCORE GEMM: 0 = the default (1024: 50 MiB of partials at
 * V = 50257), else a positive multiple of 16 (anything else: nonzero) */
int  gpt2_decode_set_score_chunk(GPT2* model, int rows);
/* Speculative greedy decoding: one pass verifies up to HPA_VERIFY_MAX_ROWS - 1
 * drafted tokens per sequence and emits what the model itself would have
 * emitted token by token -- the accepted drafts and one token of its own --
 * while reading each sequence's K/V once.
 * n_draft[b] in [-1, HPA_VERIFY_MAX_ROWS - 1]: -1 leaves sequence b untouched
 * (position, next id, logits row, sampler state, log-probability: lens[b] = 0
 * of the ragged call); 0 is a plain decode step of b through this path.
 * drafts: the drafted ids packed in sequence order (sum of the positive
 * n_draft; NULL when there are none).
 * The pass is the ragged pass over n_draft[b] + 1 rows per sequence: row 0 is
 * b's pending next id (the device's, as gpt2_decode_step(model, NULL, ..)
 * would feed it), rows 1.. its drafts; the K/V of every row is appended.  The
 * rows' greedy ids come from the SCORE GEMM (no dense logits), the accept
 * decision is taken on the device (hpa_verify_accept): a = the number of
 * leading drafts equal to the greedy id of the row before them.  Then the
 * ragged pass's tail from row a: logits GEMM and pick.
 *   n_accepted[b] = a (-1: untouched)
 *   out_tokens[b * HPA_VERIFY_MAX_ROWS + i], i <= a: the a accepted drafts,
 *     then the model's own next token (the pick: b's new pending id)
 *   draft_logprobs (nullable, same stride): entry i < n_draft[b] =
 *     log p(draft_{i+1} | pending, draft_1..i) under the raw distribution, for
 *     every drafted row, accepted or not (conditioned on the drafted prefix)
 * Afterwards pos[b] += a + 1 and the state is what a + 1 calls of
 * gpt2_decode_step(model, NULL, ..) would leave for b (gpt2_decode_logits row
 * b, and with gpt2_decode_set_logprobs on the pending token's
 * log-probability).  The slots past the new position hold the rejected rows'
 * K/V: no kernel reads them and later appends overwrite them; pages taken for
 * rejected rows stay with the sequence, as after gpt2_decode_set_positions.
 * Eviction and shared pages as in gpt2_decode_prefill_ragged.  Eager and
 * host-synchronous like the prefill; a captured decode graph stays valid.
 * Refused (message, nonzero, nothing changed): a sampling mode other than 0
 * (gpt2_decode_verify_sampled is the pass for mode 2), n_draft out of range, a draft id
 * outside [0, vocab_size), pos[b] + n_draft[b] + 1 > max_ctx, no engine.
 * The pending id must be valid: for a fresh slot or a fork of a shorter
 * prefix it is not, and that is the caller's responsibility, as with
 * tokens == NULL in gpt2_decode_step. */
int  gpt2_decode_verify(GPT2* model, const int* drafts, const int* n_draft, int* n_accepted, int* out_tokens,
                        float* draft_logprobs);
/* The attention kernel of a verify pass of at most max_rows rows per sequence,
 * pure: 1 hpa_paged_attention_verify (the decode kernel's K/V streaming, every
 * tile used for all rows), 0 hpa_paged_attention_prefill_ragged.  request: 0
 * auto, 1 the prefill kernel, 2 the verify kernel -- still refused (0) where
 * it does not apply: bf16 and fp8 pools (their tile loops are not written:
 * the prefill kernel is correct there, and slower), head size != 64, a page
 * size other than 8, 16, 32 or 64, more than HPA_VERIFY_MAX_ROWS rows. */
int  gpt2_decode_verify_plan(int max_rows, int kv_dtype, int page_size, int head_size, int request);
/* the request gpt2_decode_verify passes to the plan (default 0) */
int  gpt2_decode_set_verify_attention(GPT2* model, int request);
/* Speculative sampling: gpt2_decode_verify under sampling mode 2 (per-sequence
 * temperature / top-k / top-p).  Arguments, row layout, page growth, eviction,
 * trace arming, out_tokens layout and position bookkeeping are
 * gpt2_decode_verify's.  Drafts are point-mass proposals (exact for a
 * deterministic drafter: gpt2_ngram_draft, a greedy draft model; a sampled
 * draft model's own distribution q is not taken).  With p_i the distribution
 * mode 2 draws from at row i (hpa_sample_filtered's kept set and masses under
 * b's settings) and d_{i+1} the draft after it, rows are examined in order:
 *   - one coin u = j / 2^24 from b's stream; d_{i+1} is accepted iff
 *     u < p_i(d_{i+1}), the integer test w_target * 2^24 > w_total * j
 *     (a draft outside the kept set is always rejected, a draft that is the
 *     whole kept set always accepted);
 *   - at the first rejection, at row a, b's own token is drawn from p_a with
 *     d_{a+1} removed and the rest renormalised (hpa_sample_filtered_ex), with
 *     one more coin;
 *   - with every draft accepted the own token is a plain mode-2 draw from the
 *     last row.
 * The emitted tokens are distributed exactly as token-by-token mode-2 sampling.
 * A temperature-0 sequence is greedy (accepts iff the draft is the argmax); its
 * coins are still drawn.  b's sampler state advances examined + 1 times,
 * examined = the drafted rows up to and including the first rejection; an
 * untouched sequence advances nothing.
 * The pass: hpa_verify_rows, the layers with gpt2_decode_verify_plan's
 * attention kernel, then the drafted rows through the dense route in chunks of
 * gpt2_decode_set_score_chunk rows (default 256): one LOGITS GEMM into
 * gpt2_decode_score_top's [chunk][V] workspace and one
 * hpa_sample_filtered_prob with the drafts as targets; hpa_spec_accept; then
 * the verify pass's tail (gather, logits GEMM, pick, log-probabilities as set).
 *   draft_probs (nullable, stride HPA_VERIFY_MAX_ROWS): entry i < n_draft[b] =
 *     (float)((double)w_target / w_total) of drafted row i, for every drafted
 *     row, examined or not.
 * Refused (message, nonzero, nothing changed, sampler states included): a
 * sampling mode other than 2 (mode 0: gpt2_decode_verify; mode 1's order-exact
 * float sampler has no integer masses), logit processors on, and everything
 * gpt2_decode_verify refuses.  Buffers are allocated on first use and freed
 * with the engine. */
int  gpt2_decode_verify_sampled(GPT2* model, const int* drafts, const int* n_draft, int* n_accepted, int* out_tokens,
                                float* draft_probs);
/* n-gram (prompt-lookup) drafter, host only (no device, allocation or I/O):
 * for g from max_ngram down to min_ngram, the most recent earlier occurrence
 * of the last g tokens of history[0..n) that has at least one token after it;
 * up to k of the tokens that followed it are copied to draft.  Returns how
 * many (0: no match, k <= 0, n too short). */
int  gpt2_ngram_draft(const int* history, int n, int max_ngram, int min_ngram, int k, int* draft);
/* Tree speculation: gpt2_decode_verify over a draft TREE per sequence, greedy.
 * The n_draft[b] + 1 <= HPA_VERIFY_MAX_ROWS rows of sequence b are tree nodes:
 * node 0 is b's pending id, draft j (0-based, packed like `drafts`) is node
 * j + 1 and hangs from node parents[j] in [0, j] (`parents` is packed like
 * `drafts`; a parent is always a smaller node index than its child).  A chain
 * is parents[j] = j.  One pass verifies every branch and continues from the
 * deepest node the model agrees with; each sequence's cached K/V is read once,
 * exactly as in gpt2_decode_verify.
 * n_draft (-1 untouched, 0 a plain step), out_tokens (stride
 * HPA_VERIFY_MAX_ROWS: the a accepted tokens, then the model's own), page
 * growth, eviction, shared pages, trace arming (rows in node order) and the
 * tail (gather from the continuing row, logits GEMM, pick, log-probabilities /
 * top log-probabilities as set) are gpt2_decode_verify's.
 * The pass: hpa_verify_tree_rows (node i of b: wpe position pos[b] + depth(i),
 * K/V appended to slot pos[b] + i, ancestor mask); the layers with
 * hpa_paged_attention_verify_tree (a node sees the cached context and its own
 * ancestors, never a sibling branch); every row's greedy id from the SCORE GEMM
 * with targets -1; hpa_verify_tree_accept: cur = node 0, and while some child c
 * of cur (lowest index first) carries the greedy id of cur, cur = c; then
 * hpa_pool_compact_path moves the K/V of the accepted path's nodes into the
 * consecutive slots pos[b] + 1 .. pos[b] + a in every layer (one launch); then
 * the tail from cur's row.
 *   n_accepted[b] = a = depth(cur) (-1: untouched)
 *   out_tokens[b * HPA_VERIFY_MAX_ROWS + i], i <= a: the accepted drafts along
 *     the path, then the model's own next token (b's new pending id)
 *   accepted_nodes (nullable, same stride): entry i < a = the node index
 *     (1-based among the drafts: draft j is node j + 1) of the i-th accepted draft
 * Afterwards pos[b] += a + 1 and the engine is in the state a + 1 greedy steps
 * would leave, K/V slots included.  The slots past the new position hold
 * rejected nodes' rows, which nothing reads.
 * Limits: greedy (gpt2_decode_verify_tree_sampled is the pass for sampling
 * mode 2); fp32 KV pools (the
 * bf16 / fp8 pools' prefill kernel has no tree mask); at most
 * HPA_VERIFY_MAX_ROWS nodes; no drafted-token log-probability output (a node
 * with several children has several targets and the SCORE epilogue takes one
 * per row).
 * Refused (message, nonzero, nothing changed -- positions, pages, pending ids):
 * everything gpt2_decode_verify refuses (a sampling mode other than 0, logit
 * processors on, n_draft or a draft id out of range, overflow of max_ctx, no
 * engine), a parent outside [0, j], two siblings (same parent) with the same
 * token, and an engine for which gpt2_decode_verify_plan(rows, kv_dtype,
 * page_size, head_size, 0) != 1. */
int  gpt2_decode_verify_tree(GPT2* model, const int* drafts, const int* parents, const int* n_draft,
                             int* n_accepted, int* out_tokens, int* accepted_nodes);
/* n-gram tree drafter, host only (no device, allocation or I/O).  For g from
 * max_ngram down to min_ngram, the earlier occurrences of the last g tokens of
 * history[0..n) that have at least one token after them are scanned, most
 * recent first; each one's continuation (up to `depth` tokens) is inserted
 * into a trie rooted at node 0 (the pending token): existing prefixes are
 * shared, new nodes appended, so parents precede children.  Stops once
 * max_nodes (1..HPA_VERIFY_MAX_ROWS - 1) drafts exist -- an insertion is cut
 * there -- or once max_branches continuations have each added at least one
 * node.  draft[j] / parents[j] (room for max_nodes each): draft j's token and
 * parent node, in gpt2_decode_verify_tree's layout.  Returns the number of
 * drafts (0: no match, or max_nodes, depth or max_branches < 1, n too short).
 * The first inserted continuation is gpt2_ngram_draft's with k = depth, so for
 * depth <= max_nodes the tree's first-child chain is that draft. */
int  gpt2_ngram_draft_tree(const int* history, int n, int max_ngram, int min_ngram, int max_nodes, int depth,
                           int max_branches, int* draft, int* parents);
/* Sampled tree speculation: gpt2_decode_verify_tree under sampling mode 2.
 * Arguments and layouts are gpt2_decode_verify_tree's.  The drafts are
 * point-mass proposals (a deterministic drafter: gpt2_ngram_draft_tree, a
 * greedy draft model), siblings carry distinct tokens, and multi-draft
 * rejection sampling reduces to a rule that is exact in the sampler's
 * fixed-point integers.  With p_i the distribution mode 2 draws from at node
 * i's row (hpa_sample_filtered's kept set and masses under b's settings) and
 * S_i its kept total, the walk starts at cur = node 0:
 *   1. rem = S_cur; the children c of cur are examined in ascending node
 *      index, w_c = the mass of c's token in p_cur (0 outside the kept set);
 *   2. per child one coin j = xorshift_u32(state[b]) >> 8; c is accepted iff
 *      w_c * 2^24 > rem * j (128-bit integers): then cur = c and the walk
 *      restarts at 1; else rem -= w_c and the next child is examined;
 *   3. the walk ends when cur is a leaf or every child of cur was rejected;
 *   4. b's own token is one more mode-2 draw from p_cur with every rejected
 *      child of cur removed (total rem; hpa_sample_filtered_exn), one more coin.
 * At one node the first child c_1 is emitted with probability p(c_1); otherwise
 * the walk goes on under p with c_1 removed and renormalised, which is where a
 * token-by-token draw that did not give c_1 stands: by induction over the
 * children the emitted token is distributed as p, and over the depth the
 * emitted sequence as token-by-token mode-2 sampling.  A rejected child has
 * w_c < rem, so rem > 0 throughout; a child that is the whole remaining kept
 * set is always accepted; a temperature-0 sequence accepts exactly the child
 * that carries the greedy id (its coins are still drawn).  b's sampler state
 * advances once per examined child and once for its own token.  A chain
 * (parents[j] = j) is exactly gpt2_decode_verify_sampled.
 * The pass: hpa_verify_tree_rows; the layers with the tree attention kernel;
 * the internal nodes (those with a child: gpt2_tree_dense_tables) through the
 * dense route in chunks of gpt2_decode_set_score_chunk rows -- one LOGITS GEMM
 * into the [chunk][V] workspace and one hpa_sample_filtered_prob_multi, each
 * internal node once however many children it has, so that all of them are
 * judged against one total; hpa_spec_tree_accept; hpa_pool_compact_path; then
 * the tail from cur's row (gather, logits GEMM, hpa_sample_filtered_exn,
 * log-probabilities / top log-probabilities as set).  As in the chain pass the
 * accept decision reads the dense route's row and the pick recomputes its
 * masses from the tail's row.
 *   draft_probs (nullable, stride HPA_VERIFY_MAX_ROWS): entry j < n_draft[b] =
 *     (float)((double)w_j / S_parent(j)): draft j's unconditional mass at its
 *     parent's row, for every draft, examined or not.
 * Afterwards pos[b] += a + 1 and the K/V slots are those of a + 1 mode-2 steps.
 * Refused (message, nonzero, nothing changed -- positions, pages, pending ids,
 * sampler states): a sampling mode other than 2, logit processors on, and
 * everything gpt2_decode_verify_tree refuses otherwise.  Buffers are allocated
 * on first use and freed with the engine. */
int  gpt2_decode_verify_tree_sampled(GPT2* model, const int* drafts, const int* parents, const int* n_draft,
                                     int* n_accepted, int* out_tokens, int* accepted_nodes, float* draft_probs);
/* The tables of that pass's dense route, host only (no device, allocation or
 * I/O).  drafts / parents / n_draft: gpt2_decode_verify_tree's (a parent
 * outside [0, j] is clamped into it); row0[b]: sequence b's first packed row
 * (node i of b is row row0[b] + i).  Per internal node -- a node with at least
 * one child -- in (sequence, node) order: rows[k] its packed row, seq[k] its
 * sequence, targets[k * 7 ..] its children's tokens in ascending child order,
 * n_targets[k] their number, dst[k * 7 ..] each child's index as a packed
 * draft (draft j of b: the drafts before b's, plus j); unused entries -1.
 * rows, seq and n_targets need room for one entry per draft, targets and dst
 * for 7.  Returns the number of internal nodes (at most the number of drafts).
 * This is the one place that decides which rows reach the LOGITS GEMM: each
 * internal node once, however many children it has. */
int  gpt2_tree_dense_tables(const int* drafts, const int* parents, const int* n_draft, int B, const int* row0,
                            int* rows, int* seq, int* targets, int* n_targets, int* dst);
/* enable != 0: every pick (decode step, prefill, ragged prefill, score) is
 * followed by one hpa_logprob_rows launch: the log-probability of the chosen
 * id under the raw model distribution (temperature 1, no filter, in every
 * sampling mode) into a device [B] array; sequences a ragged call leaves
 * untouched keep their value.  Default off: the step's launches are then
 * exactly those without it.  Toggling drops a captured graph. */
int  gpt2_decode_set_logprobs(GPT2* model, int enable);
/* host_out [B] <- those log-probabilities (waits for the queued work);
 * host_out NULL: only the status.  Nonzero unless gpt2_decode_set_logprobs is on. */
int  gpt2_decode_logprobs(GPT2* model, float* host_out);
/* top log-probabilities (the alternatives: `top_logprobs` of the OpenAI API).
 * k in [0, HPA_TOP_LOGPROBS_MAX]; 0 = off (default).  While on, every pick (decode
 * step, prefill, ragged prefill, score, the tail of a verify pass) is followed
 * by one hpa_top_logprobs pass over the raw logits rows [B][V]: the raw model
 * distribution whatever the sampling mode, filters or logit processors, like
 * gpt2_decode_logprobs.  Entry j of a row is the j-th column under (logit
 * descending, column ascending on equal logits).  Rows a ragged call leaves
 * untouched keep their values; a change of k clears every row to zeros until a
 * pick rewrites it.  Changing k drops a captured graph; k out of range:
 * nonzero, message, nothing changed.  Buffers allocated on first enable, freed
 * with the engine. */
int  gpt2_decode_set_top_logprobs(GPT2* model, int k);
int  gpt2_decode_top_logprobs_k(GPT2* model);              /* -1 without an engine */
/* host [B][k] each (either nullable); waits for queued work; nonzero while off */
int  gpt2_decode_top_logprobs(GPT2* model, int* ids, float* logprobs);
/* gpt2_decode_score, and for every packed row r the k best columns and their
 * log-probabilities: top_ids / top_lps host [sum(lens)][k].  logprobs / targets
 * as in gpt2_decode_score (targets required; -1 = none).  k in [1, HPA_TOP_LOGPROBS_MAX].
 * The SCORE epilogue keeps one maximum per 16-column tile, so this call takes
 * the dense route in chunks: per chunk of gpt2_decode_set_score_chunk rows
 * (default here 256: 51 MB at V = 50257) one LOGITS GEMM into a [chunk][V]
 * workspace (allocated on first use, freed with the engine) and one
 * hpa_top_logprobs with the chunk's targets.  Everything else is the ragged
 * pass.  Bad k, a target outside [-1, vocab_size) or a null output: nonzero,
 * nothing changed. */
int  gpt2_decode_score_top(GPT2* model, const int* tokens, const int* lens, const int* targets, float* logprobs,
                           int k, int* top_ids, float* top_lps, int* next_tokens);
/* retire sequence seq: its pages go back to the pool (block_manager.c:78-90),
 * its position restarts at 0, so the slot can admit a new prompt.  The slot's
 * sampler state and sampling settings (gpt2_decode_set_sampling_params) stay
 * as they are */
int  gpt2_decode_release(GPT2* model, int seq);
/* prefix sharing: sequence dst continues from the first n_tokens cached tokens
 * of sequence src (n_tokens in [1, pos[src]], or -1 for pos[src]) without
 * computing or storing them again -- one system prompt for many requests, or N
 * samples of one prompt.  dst must be fresh or released (position 0, no
 * pages).  Any violation, src == dst and a sequence out of range included,
 * returns nonzero with a message and changes nothing.
 * dst shares src's n_tokens / P full pages (bm_fork_prompt: one more holder
 * each, nothing copied); when n_tokens % P != 0 it takes ONE fresh page and the
 * partly filled page is copied into it in every layer by one launch
 * (hpa_pool_copy_pages; the slots beyond n_tokens carry stale bytes no kernel
 * reads, as in any reused page).  pos[dst] = n_tokens.  When n_tokens ==
 * pos[src], dst also inherits src's pending next id, so gpt2_decode_step(model,
 * NULL, ...) continues both; otherwise dst has no valid next id until it is fed
 * tokens.  dst's sampler state and sampling settings are untouched (seeded
 * seed + dst), so forks of one prompt draw different tokens.  Only full pages are shared and the tail
 * is copied here, so appends after a fork land in private pages; a sequence
 * rewound into a shared page (gpt2_decode_set_positions) gets a private copy
 * of it before its next append.  The LRU policy never evicts the holder of a
 * shared page for that page (block_manager.h); if the fresh page's allocation
 * pages out src itself the call fails.  Releasing or evicting one holder
 * leaves the pages to the others.  gpt2_decode_fill_random* refuses while
 * pages are shared.  Waits for queued work like gpt2_decode_release. */
int  gpt2_decode_fork(GPT2* model, int src, int dst, int n_tokens);
/* ---------------- parking: preemption by swap ----------------
 * gpt2_decode_park copies everything that belongs to sequence seq at position
 * n = pos[seq] >= 1 into host memory and returns a handle; gpt2_decode_unpark
 * puts a handle into a fresh or released slot, which then is in the state the
 * parked sequence was in: gpt2_decode_step(model, NULL, ..) continues it bit
 * for bit and every per-sequence readback returns what it returned before the
 * park.  The other answer to a full pool besides the LRU eviction (a sequence
 * thrown away and prefilled again), and a way to set an idle conversation aside.
 *
 * park waits for queued work like gpt2_decode_release, then copies:
 *   - the K/V: the ceil(n / P) pages of every layer into ONE pinned host
 *     allocation, by hpa_pool_gather_pages writing straight into it (layout:
 *     hpa_park_offset).  The partly filled last page travels whole (its slots
 *     past n hold bytes no kernel reads, as in any reused page); shared pages
 *     are read like any others;
 *   - the device words d_next[seq], d_tokens[seq] and, once
 *     gpt2_decode_set_sampling was called, the sampler state;
 *   - the readback rows: the logits row [V] and, where the feature is on, the
 *     processed-logits row, the pending id's log-probability, the top
 *     log-probability row (ids and values, k of them);
 *   - the settings: temperature / top-k / top-p, the penalties, from_pos, the
 *     bias list;
 *   - with processors on the recorded history [0, n);
 *   - the geometry: kv dtype, P, num_layers, num_heads, head_size, vocab_size,
 *     and of an fp8 pool the 2 * L * NH K/V scales.
 * keep == 0: the slot is then released exactly as gpt2_decode_release does it
 * (only after the copy has completed).  keep != 0: the sequence stays live and
 * untouched -- a checkpoint.  No engine, seq out of range, pos[seq] == 0 or a
 * failed allocation: NULL with a message, nothing changed.
 *
 * unpark: the target must be fresh or released (position 0, no pages), as for
 * gpt2_decode_fork.  Refused -- message, nonzero, no page, position, setting or
 * device word changed -- when the target is live or out of range; when a
 * geometry field differs (on fp8: a scale, bit for bit); when n > max_ctx; when
 * processors are on in the engine and the handle carries no history; when
 * gpt2_decode_free_pages() < ceil(n / P).  An unpark never evicts anyone: the
 * caller parks someone else first.  On success the slot takes ceil(n / P)
 * private pages, the payload is scattered into them (hpa_pool_scatter_pages),
 * every word, row and setting above is restored (with processors on: the
 * history uploaded and the counts recounted over the slot's window), pos[seq]
 * = n.  A row of a feature that was off at the park and is on now is left as
 * it is until the next pick rewrites it.  A captured decode graph stays valid:
 * everything it reads is a device array.  Waits for its copies.
 * The handle is host memory only and is not consumed: unparking it into two
 * slots is a host-level fork, and it may go into another engine of the same
 * geometry.  gpt2_parked_tokens: n; gpt2_parked_bytes: the K/V payload
 * (hpa_park_bytes); gpt2_parked_free(NULL) is fine. */
typedef struct GPT2Parked GPT2Parked;
GPT2Parked* gpt2_decode_park(GPT2* model, int seq, int keep);
int    gpt2_decode_unpark(GPT2* model, const GPT2Parked* parked, int seq);
int    gpt2_parked_tokens(const GPT2Parked* parked);
size_t gpt2_parked_bytes(const GPT2Parked* parked);
void   gpt2_parked_free(GPT2Parked* parked);
/* ---------------- shared-prefix attention ----------------
 * Forks of one prefix hold the same pages for it, and the decode attention
 * still streams them once per sequence.  With this on (default off) the decode
 * attention streams the leading 64-token tiles that a unit of up to
 * HPA_SHARED_MAX_ROWS sequences hold in the same pages ONCE per unit
 * (hpa_paged_attention_decode_shared, hip_paged_attn.h): a prefix launch and a
 * suffix launch wherever the decode attention is its own launch (the five-launch
 * loop and every form whose plan has attn_launch = 1, traced steps and
 * gpt2_decode_time_attention included).  Outputs are the plain step's within
 * fp32 rounding (another summation grouping); a sequence outside every unit
 * gets the plain kernel's bits, and while no unit exists the step is the plain
 * step, launch for launch.
 *
 * The plan, pure (no device, allocation or global).  block_table [B][bt_stride]:
 * page ids, -1 for none; pos[b]: b's cached tokens.  common(a, b) = the
 * leading i with bt[a][i] == bt[b][i] >= 0; share(a, b) = min(common *
 * page_size, pos[a], pos[b]) / 64, whole 64-token tiles.
 *   1. unassigned = every b with pos[b] >= 64, in index order;
 *   2. the leader a = the lowest unassigned index;
 *   3. its candidates = the unassigned b > a with share(a, b) >= min_tiles,
 *      by share descending, then index ascending;
 *   4. for k = 1 .. min(7, candidates), t_k = the k-th candidate's share: the
 *      k with the largest k * t_k, the larger k on a tie;
 *   5. k + 1 >= min_members: the unit (a, the first k candidates, tiles = t_k)
 *      is emitted and its members leave the set; else a leaves alone;
 *   6. from 2 until the set is empty.
 * unit_members [max_units][HPA_SHARED_MAX_ROWS] (-1 padded), unit_tiles
 * [max_units] (0 = unused), seq_skip[b] = the tiles of b's unit, else 0.
 * Every unit: members pairwise identical in every page covering tokens
 * [0, 64 * tiles), 64 * tiles <= pos[m] for each member, a sequence in at most
 * one unit.  Returns the number of units; < 0 for a null pointer, B,
 * bt_stride or page_size < 1, min_tiles < 1, min_members < 2 or max_units <
 * B / 2. */
int  gpt2_attn_shared_plan(const int* block_table, int bt_stride, const int* pos, int B, int page_size,
                           int min_tiles, int min_members, int max_units, int* unit_members, int* unit_tiles,
                           int* seq_skip);
/* 1 on, 0 off (default).  Refused on a bf16 or fp8 pool (message, nonzero,
 * nothing changed).  Toggling drops a captured graph.  The engine rebuilds
 * its plan only while pages are shared and only after gpt2_decode_fork,
 * gpt2_decode_release, gpt2_decode_reset, an eviction, a copy-on-write,
 * gpt2_decode_set_positions or this call -- never in a plain step: appends add
 * private pages at the end and positions only grow, so a plan stays valid
 * across steps, prefill and verify passes (which are unchanged).  The tables
 * are sized for B / 2 units and uploaded through pinned staging; a plan change
 * keeps the graph unless it goes between no unit and some unit or changes the
 * prefix launch's ranges (hpa_attn_shared_pick_splits).  Forms that run the
 * attention inside a persistent launch (A/B builds) do not take it. */
int  gpt2_decode_set_shared_attention(GPT2* model, int enable);
int  gpt2_decode_shared_attention(GPT2* model);
/* the plan in use: unit_of[b] = b's unit or -1, shared_tokens[b] = the tokens
 * its unit streams for it (each nullable, [B]).  Returns the units (0 while
 * off, while nothing is shared, or while the units cover fewer than
 * min_covered sequences), -1 without an engine. */
int  gpt2_decode_shared_plan(GPT2* model, int* unit_of, int* shared_tokens);
/* the plan's min_tiles (>= 1) and min_members (>= 2), and min_covered (>= 2):
 * a plan whose units hold fewer sequences than that is not used (no unit:
 * the plain step).  The defaults are the measured ones, 15 / 2 / 64 (README
 * "Shared-prefix attention": the two launches beat the one only where the
 * whole batch of 64 shares long prefixes).  Takes effect at the next step. */
int  gpt2_decode_set_shared_thresholds(GPT2* model, int min_tiles, int min_members, int min_covered);
int  gpt2_decode_shared_thresholds(GPT2* model, int* min_tiles, int* min_members, int* min_covered);
/* the prefix launch's ranges per (unit, head): 0 (default) by shape
 * (hpa_attn_shared_pick_splits), else 1..HPA_ATTN_MAX_SPLITS (timing tools);
 * takes effect at the next step.  And the value of the plan in use. */
int  gpt2_decode_set_shared_splits(GPT2* model, int splits);
int  gpt2_decode_shared_splits(GPT2* model);
/* free pages of the engine's manager (-1 without an engine) */
int  gpt2_decode_free_pages(GPT2* model);
/* where the engine keeps the manager's pages: out[i] = the pool slot (the page
 * index of hip_paged_attn.h's pool layout) of manager page i, for i < n.  The
 * map is a fixed permutation chosen at gpt2_decode_init.  Returns the number
 * of entries written (min(n, the manager's max_blocks)), -1 without an engine. */
int  gpt2_decode_page_slots(GPT2* model, int* out, int n);
/* the same, but enqueue only (no host sync; next ids stay on device) */
int  gpt2_decode_step_async(GPT2* model, const int* tokens);
/* one eager step that also copies the residual stream entering every layer
 * and the final one to host_x, row-major [L+1][B][C] (per-layer parity tests) */
int  gpt2_decode_step_traced(GPT2* model, const int* tokens, int* next_tokens, float* host_x);
/* the same for the dense ragged pass: arms the next call of
 * gpt2_decode_prefill / _prefill_ragged / _score / _score_top / _verify, and
 * that call only (it disarms on every exit path, refusals included;
 * gpt2_forward's window prefill is such a pass too and uses it up).  The pass
 * copies its residual stream after the embedding and after every layer to
 * host_x, row-major [L+1][R][C], R the pass's packed rows in their order.
 * floats: the room at host_x; a pass that needs more is refused before it
 * changes anything (no page, no position).  host_x NULL disarms.  Off (the
 * default) adds no launch. */
int  gpt2_decode_trace_next_pass(GPT2* model, float* host_x, size_t floats);
/* free every sequence's pages and rewind positions to 0 */
int  gpt2_decode_reset(GPT2* model);
/* synthetic K/V for positions [0, ctx) of every sequence (benchmark prefill) */
int  gpt2_decode_fill_random(GPT2* model, int ctx, unsigned long long seed);
/* the same with the K/V of global sequences seq_offset.. (a shard of a larger
 * batch gets exactly its rows of the unsharded fill) */
int  gpt2_decode_fill_random_ex(GPT2* model, int ctx, unsigned long long seed, int seq_offset);
/* allocate the pages of positions [0, ctx) up front (no host work per step) */
int  gpt2_decode_reserve(GPT2* model, int ctx);
/* rewind/advance positions (pages kept) */
int  gpt2_decode_set_positions(GPT2* model, const int* pos);
/* capture the step into a hipGraph and replay it (1) or launch eagerly (0) */
int  gpt2_decode_set_graph(GPT2* model, int enable);
/* context ranges per (sequence, head) of the decode attention
 * (hpa_paged_attention_decode_split): 0 = by shape (hpa_attn_pick_splits:
 * GPT-2 124M 1 at B >= 64 and 16, 2 at 32 and 8), else 1..16 */
int  gpt2_decode_set_attn_splits(GPT2* model, int splits);
int  gpt2_decode_attn_splits(GPT2* model);
/* waves per attention workgroup the engine picked for its batch (hpa_attn_pick_waves) */
int  gpt2_decode_attn_waves(GPT2* model);
/* the layer loop's form, as a request 0..7 (clamped): 0 five launches per
 * layer; 1 (default, "auto") the form measured fastest (profiles/r4: 5 at
 * C = 768, 6 at C >= 1024, else 3); 2 one persistent launch per layer
 * (hpa_decode_layer: attention -> attproj -> fc -> fcproj -> next qkv); 3 the
 * decode attention's own launch + one persistent launch of the GEMM chain
 * (attproj -> fc -> fcproj -> next qkv) in 4-wave units; 4 the chain in round
 * 3's wide units (C = 768, else 3); 5 chain form 6: every phase in 12-wave
 * units of T tiles, one per workgroup, 16-byte epilogues, waits per row block
 * (C = 768, else 3); 6 chain form 8: streamed-weight units for MFMA-bound
 * wide layers (C = 768 / 1024 / 1280 / 1600: GPT-2 124M to XL); 7 the
 * pipelined halves (hpa_decode_pipe, hpa_pipe.hip): the step's first launch,
 * ONE persistent launch of every layer with the batch in two halves (the GEMM
 * chain of one half on g_cus CUs beside the attention of the other on the
 * rest), the logits; bit-identical to 5, which runs where they do not apply
 * (they need GPT-2 124M shapes, fp32 weights and pool, 17..64 rows) and in
 * traced steps.  2, 4 and 7 are in A/B builds (-DHPA_AB) only: the product
 * build runs five launches for 2 and 4, and 5 for 7.  With bf16 weights every
 * request but 0 is the bf16-weight chain (C = 768, B <= 256); with an fp8 pool
 * only 1 and 5 leave five launches (gpt2_decode_init_ex).  A request that
 * does not apply to the shape or the device runs five launches.  What a
 * request becomes is decided by gpt2_decode_layer_plan alone.
 * HPA_LAYER_KERNEL=0..7 in the environment sets the default.  A persistent
 * launch needs every CU for its 12-wave workgroups: a GPU shared with another
 * process's persistent kernels should use 0. */
int  gpt2_decode_set_layer_kernel(GPT2* model, int enable);
/* CUs of the pipelined halves' GEMM role (multiple of 8; 0: the default, 64) */
int  gpt2_decode_set_pipe_split(GPT2* model, int g_cus);
/* the form in use (the plan's `form`): 0 five launches, 1 full persistent
 * layer, 2 attention launch + persistent chain of 4-wave units, 3 attention
 * launch + the chain in wide / multi-tile / streamed-weight units (requests
 * 4..6, and 7 where the halves do not apply), 4 the bf16-weight chain, 5 the
 * pipelined halves */
int  gpt2_decode_layer_kernel(GPT2* model);
/* The plan of a decode step's layer loop: the one function that decides what
 * a request becomes, pure (every input by value; no device, allocation or
 * global), so every routing rule can be checked without a GPU.  request 0..7
 * as gpt2_decode_set_layer_kernel; B the engine's batch (eligibility) and
 * pick_B the batch its shape picks follow (gpt2_decode_set_global_batch, else
 * B); kv_dtype HPA_F32 / HPA_BF16 / HPA_FP8; w_bf16 1 for bf16 weights (fp32
 * weights are taken to have their LN-fold pack, as gpt2_decode_init* makes
 * it); num_cus the device's CU count (hpa_device_info).  out5:
 *   [0] form         what gpt2_decode_layer_kernel reports (0..5, above)
 *   [1] chain        HpaLayerArgs.chain_only of forms 1..3, 5 (0, 1, 2..6, 8)
 *   [2] splits       attention ranges inside the layer launch (1 unless form 1)
 *   [3] first        the step's first launch: 0 the embed kernel (+ the qkv(0)
 *                    GEMM), 1 hpa_decode_first, 2 hpa_decode_chain_b16_first
 *   [4] attn_launch  1: the decode attention is its own launch before each
 *                    layer launch (forms 2..5)
 * Returns 0 (1: out5 NULL).  The answer is the build's: an A/B build also
 * yields forms 1 and 5 and chains 2..5. */
int  gpt2_decode_layer_plan(int request, int B, int pick_B, int C, int num_heads, int max_ctx, int kv_dtype,
                            int w_bf16, int num_cus, int out5[5]);
/* waits for the queued work; 0, or the code of a timed-out in-launch wait of
 * the persistent layer (the step's outputs are then invalid), which it clears */
int  gpt2_decode_status(GPT2* model);
/* attention-kernel timing with HIP events around every layer's attention
 * launch (forces eager launches while enabled) */
int    gpt2_decode_profile(GPT2* model, int enable);
double gpt2_decode_profile_read(GPT2* model, long* launches);
/* device buffers: logits [B][V], next ids [B]; host positions [B]; batch */
float* gpt2_decode_logits(GPT2* model);
int*   gpt2_decode_next(GPT2* model);
int    gpt2_decode_positions(GPT2* model, int* host_pos);
int    gpt2_decode_batch(GPT2* model);
/* sequences the LRU policy paged out since the last call (block_manager.c:
 * 104-113 evicts a whole sequence when the pool is full; it restarts at
 * position 0 and must be prefilled again); mask (nullable, [B]) marks them.
 * Returns how many. */
int    gpt2_decode_evicted(GPT2* model, int* mask);
/* fp8 pools (HPA_FP8): the per-head scales of K and V, host arrays
 * [num_layers][num_heads], every entry finite and > 0.  A value x is stored
 * as the e4m3fn code of clamp(x / scale, +-448) and read back as
 * decode(code) * scale.  Nonzero on an fp32 / bf16 engine, on a bad scale, and
 * unless every sequence is at position 0 (a fresh engine, or after
 * gpt2_decode_reset): cached codes would change their meaning.  A captured
 * graph stays valid (the kernels read the scales from device memory).
 * Calibration is the caller's job: the per-head max |K| and max |V| of
 * gpt2_decode_read_kv on an fp32-pool run, divided by 448. */
int    gpt2_decode_set_kv_scales(GPT2* model, const float* k_scale, const float* v_scale);
/* the scales in use (either array may be NULL); nonzero on a non-fp8 engine */
int    gpt2_decode_kv_scales(GPT2* model, float* k_scale, float* v_scale);
/* K/V of positions [0, n) of sequence b at layer l, token-major [n][C] host
 * arrays (the reference page layout, block_manager.c:145-146); bf16 / fp8
 * pools: the values the stored codes stand for (fp8: decode(code) * scale) */
int    gpt2_decode_read_kv(GPT2* model, int layer, int b, int n, float* k, float* v);
/* fused GEMM launch shapes [qkv, attproj, fc, fcproj, logits]: waves per
 * workgroup (4/8/16), 16-row blocks (1/2/4) and 16-column tiles (1/2/4) per
 * workgroup.  set = 0 copies them out; set = 1 applies the nonzero entries
 * (NULL = keep).  Invalid combinations fail at the next step's launch. */
int    gpt2_decode_gemm_config(GPT2* model, int* waves5, int* row_blocks5, int* col_tiles5, int set);
/* attention kernel timed alone: `iters` back-to-back launches on the engine's
 * pool at the last step's positions; average ms and algorithmic bytes per
 * launch (bench.py roofline) */
int    gpt2_decode_time_attention(GPT2* model, int iters, double* ms_per_launch,
                                  double* bytes_per_launch);
/* Infinity-Cache probe: the first `frac` of layer l's pool slab read by
 * hpa_l3_prefetch (pf_grid workgroups), then layer l's attention; average ms
 * of each part (per-iteration events) */
int    gpt2_decode_time_attention_pf(GPT2* model, int iters, double frac, int pf_grid, double* ms_attn,
                                     double* ms_pf);
/* token choice: 0 = greedy argmax (default); 1 (and any nonzero value but 2)
 * = multinomial sampling as the reference driver (softmax_forward +
 * sample_mult with random_f32 coins); 2 = filtered: temperature / top-k /
 * top-p per sequence (hpa_sample_filtered states the rules), same coins.
 * Sequence b is seeded with seed + b; the coins stay on the device */
int    gpt2_decode_set_sampling(GPT2* model, int enable, unsigned long long seed);
/* mode 2's settings of sequence seq in [0, B), or of every sequence (seq =
 * -1).  Valid: temperature finite and >= 0 (0 = greedy for that sequence),
 * top_k >= 0 (0 = off), 0 < top_p <= 1 (1 = off); anything else returns
 * nonzero with a message and changes nothing.  Defaults 1, 0, 1.  They live in
 * device arrays the kernel reads, so changing them keeps the captured graph;
 * they can be set in any mode and only mode 2 reads them.  Waits for queued
 * work like gpt2_decode_release.  gpt2_decode_release, gpt2_decode_fork and
 * eviction leave a slot's settings and sampler state untouched. */
int    gpt2_decode_set_sampling_params(GPT2* model, int seq, float temperature, int top_k, float top_p);
/* the settings of sequence seq (each out pointer nullable); nonzero for seq
 * out of range */
int    gpt2_decode_sampling_params(GPT2* model, int seq, float* temperature, int* top_k, float* top_p);
/* restart sequence seq's coin stream at seed, so a request admitted into a
 * released slot draws a reproducible stream of its own.  Nonzero before any
 * gpt2_decode_set_sampling call (no states yet) and for seq out of range.
 * Waits for queued work. */
int    gpt2_decode_seed_sequence(GPT2* model, int seq, unsigned long long seed);
/* sequence seq's sampler state as it stands (what gpt2_decode_park carries
 * along); nonzero before any gpt2_decode_set_sampling call and for seq out of
 * range.  Waits for queued work. */
int    gpt2_decode_sampler_state(GPT2* model, int seq, unsigned long long* state);
/* ---------------- logit processors ----------------
 * Repetition (CTRL / HF rule), presence and frequency (OpenAI rule) penalties
 * and a logit bias, per sequence, applied on the device before every pick.
 * Off by default; while off a step's launches and bits are what they were.
 *
 * While on, the engine keeps on the device a history int32 [B][max_ctx]
 * (history[b][p]: the token whose K/V sits at position p) and a count table
 * uint16 [B][V]: count[b][t] = the positions p in [from_pos[b], pos[b]) with
 * history[b][p] == t.  A token is recorded when it is FED: the decode step's
 * token (uploaded or fed back on the device) and every row of a prefill /
 * ragged / score pass; the pending id is not counted until it is fed.  So at
 * pick time the window holds every token fed so far, this pass's included.
 *
 * The processed logit of an active row b, column t (x = raw logit, c =
 * count[b][t]), in fp32 in this order (hpa_logits_process):
 *     if c > 0:  x = x > 0 ? x / repetition : x * repetition
 *     x = x - frequency * (float)c - (c > 0 ? presence : 0)
 *     if t is in b's bias list:  x = x + bias            (-inf: a hard ban)
 * Neutral settings (1, 0, 0, no bias) give the raw row bit for bit.  Every
 * mode then picks from the processed row: mode 0 its argmax (lowest index on
 * ties; 0 for a row with nothing above -inf), mode 1 hpa_sample_final, mode 2
 * hpa_sample_filtered (temperature and filters after the processors, as vLLM /
 * HF do; a banned id has probability 0).  The raw logits stay raw:
 * gpt2_decode_logits, gpt2_decode_logprobs and gpt2_decode_score's outputs keep
 * their meaning; the processed rows are gpt2_decode_processed_logits.  A ragged
 * call's lens[b] = 0 row keeps its processed row, counts and next id.
 *
 * gpt2_decode_release, gpt2_decode_reset and an LRU eviction zero the
 * sequence's counts (settings stay, like the sampling settings);
 * gpt2_decode_fork gives dst history[src][0..n) counted over dst's own from_pos;
 * gpt2_decode_set_positions recounts a moved sequence and refuses a position
 * above the recorded history; gpt2_decode_fill_random* and gpt2_decode_verify
 * are refused while on (each: message, nonzero, nothing changed).
 *
 * gpt2_decode_set_processors(1) needs every sequence at position 0 (a fresh
 * engine or after gpt2_decode_reset) and max_ctx <= 65535; toggling drops a
 * captured graph.  Buffers are allocated on first enable ((6 V + 4 max_ctx) B
 * bytes) and freed with the engine. */
int    gpt2_decode_set_processors(GPT2* model, int enable);
int    gpt2_decode_processors(GPT2* model);
/* sequence seq's penalties, or every sequence's (seq = -1).  Valid: repetition
 * finite and > 0 (1 = off), presence and frequency finite (0 = off), 0 <=
 * from_pos <= max_ctx (the window's first position: 0 counts the prompt as HF
 * does, the prompt length counts generated tokens only as OpenAI does);
 * anything else returns nonzero with a message and changes nothing.  The
 * settings live in device arrays, so the captured graph stays; they may be set
 * while processors are off.  Changing from_pos recounts the sequence.  Waits
 * for queued work. */
int    gpt2_decode_set_penalties(GPT2* model, int seq, float repetition, float presence, float frequency,
                                 int from_pos);
/* each out pointer nullable; nonzero for seq out of range */
int    gpt2_decode_penalties(GPT2* model, int seq, float* repetition, float* presence, float* frequency,
                             int* from_pos);
/* replaces sequence seq's (-1: every sequence's) whole bias list; n = 0 clears
 * it.  Valid: 0 <= n <= HPA_LOGIT_BIAS_MAX (300), ids distinct and in [0, V),
 * values finite or -inf (NaN and +inf refused); else nonzero, a message,
 * nothing changed.  Keeps the captured graph; waits for queued work. */
int    gpt2_decode_set_logit_bias(GPT2* model, int seq, const int* ids, const float* values, int n);
/* ids, values: room for HPA_LOGIT_BIAS_MAX entries (each nullable); *n entries are written */
int    gpt2_decode_logit_bias(GPT2* model, int seq, int* ids, float* values, int* n);
/* the processed rows, device [B][V]; NULL while processors are off */
float* gpt2_decode_processed_logits(GPT2* model);
/* readbacks (nonzero while off): the *n = pos[seq] recorded tokens of seq
 * (host_tokens nullable: only n), and its counts as ints [V] */
int    gpt2_decode_history(GPT2* model, int seq, int* host_tokens, int* n);
int    gpt2_decode_token_counts(GPT2* model, int seq, int* host_counts);
/* algorithmic HBM bytes one step reads+writes at the current positions
 * (SURVEY.md 8d formula) and the attention kernel's share of them */
double gpt2_decode_step_bytes(GPT2* model, double* attention_bytes);

/* ---------------- sequence-sharded decode ----------------
 * One process per GPU: every rank runs its own engine (gpt2_decode_init with
 * its B_local sequences, private page pool, replicated weights); nothing is
 * exchanged inside a step.  After hpa_comm_init (hip_paged_attn.h),
 * gpt2_decode_shard tells the engine every rank's row count (rank order) and
 * the root; gpt2_decode_gather then enqueues the end-of-step RCCL gather of
 * the logits (what = 0) or greedy ids (what = 1) on a communication stream
 * (double-buffered: it overlaps the next step).  gpt2_decode_gathered (root)
 * returns the device rows of the last gather after gpt2_decode_gather_wait. */
/* the batch the shape picks follow (attention splits / waves, layer-loop
 * form, logits form): 0 (default) the engine's own B -- a shard computes what
 * a single-GPU engine of its rows computes; total > 0 (<= 64 applies with
 * fp32 weights, <= 256 with bf16 weights -- the bf16 chain's row limit --
 * above that the own B) -- what the unsharded engine of `total` rows computes, bit
 * for bit.  No communicator needed.  Replaces the global-batch picks
 * gpt2_decode_shard forced until round 3. */
int    gpt2_decode_set_global_batch(GPT2* model, int total);
/* the value set by gpt2_decode_set_global_batch (0: own B), -1 without an engine */
int    gpt2_decode_global_batch(GPT2* model);
int    gpt2_decode_shard(GPT2* model, const int* rows_per_rank, int root);
int    gpt2_decode_gather(GPT2* model, int what);
/* the single-process form (hpa_comm_init_all): models[i] on device i, every
 * gather posted inside one NCCL group */
int    gpt2_decode_gather_all(GPT2** models, int n, int what);
int    gpt2_decode_gather_wait(GPT2* model);
void*  gpt2_decode_gathered(GPT2* model, int what);
void   gpt2_decode_free(GPT2* model);

#ifdef __cplusplus
}
#endif
#endif
