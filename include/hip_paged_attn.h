/*
 * hip_paged_attn.h -- C-ABI of the MI355X (gfx950) paged-attention decode
 * library libpaged_hip.so.  Plain pointers and sizes only.
 *
 * Two families of entry points:
 *
 *  hpa_*            MI355X-native building blocks of the decode step
 *                   (device memory, page pool, fused kernels).  Called by
 *                   paged_infer.c's decode driver (gpt2_decode_*), which is
 *                   the replacement for the reference's gpt2_forward
 *                   (paged_infer.c:575-729 of mx60s/llm.c-paged).
 *  reference-named  the drop-in functions of the reference's
 *                   paged_infer.c / block_manager.c API, declared in
 *                   paged_infer.h and block_manager.h.
 *
 * Error convention (reference: stderr + NULL from the allocator,
 * block_manager.c:117,139,149; exit(1) with location for device errors like
 * cudaCheck, train_gpt2.cu:27-34): hpa_* return 0 on success and a nonzero
 * code after printing "[hpa] <file>:<line> <error>" to stderr; with
 * HPA_FATAL=1 in the environment they exit(1) instead.
 *
 * Device pointers passed to hpa_* kernels must live in device-accessible
 * memory (hpa_malloc / hpa_malloc_managed / hipHostMalloc).  All launches go
 * to the library's current stream (hpa_set_stream) and are asynchronous.
 */
#ifndef HIP_PAGED_ATTN_H
#define HIP_PAGED_ATTN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- device, stream, memory, events ---------------- */
int   hpa_init(int device);            /* select device, create the default stream */
int   hpa_device_count(void);
int   hpa_get_device(void);
int   hpa_set_stream(void* hip_stream); /* NULL = library default stream */
void* hpa_get_stream(void);
int   hpa_synchronize(void);            /* stream sync */
int   hpa_device_synchronize(void);
void* hpa_malloc(size_t bytes);          /* hipMalloc; NULL on failure */
void* hpa_malloc_managed(size_t bytes);  /* hipMallocManaged (host-dereferenceable) */
void* hpa_host_alloc(size_t bytes);      /* pinned host memory */
int   hpa_free(void* p);
int   hpa_host_free(void* p);
int   hpa_memcpy(void* dst, const void* src, size_t bytes);       /* hipMemcpyDefault, sync */
int   hpa_memcpy_async(void* dst, const void* src, size_t bytes); /* on the current stream */
int   hpa_memset_async(void* dst, int value, size_t bytes);
/* read [p, p + bytes) on the current stream and drop it, so a later kernel
 * finds those lines in the 256 MiB Infinity Cache (grid: workgroups of 256) */
int   hpa_l3_prefetch(const void* p, size_t bytes, int grid);
int   hpa_is_device_accessible(const void* p); /* 1 if a kernel may dereference p */
void* hpa_event_create(void);
int   hpa_event_record(void* ev);
float hpa_event_elapsed_ms(void* start, void* stop); /* syncs on stop */
int   hpa_event_destroy(void* ev);
void* hpa_event_create_nt(void);          /* no timing: fork/join ordering only */
int   hpa_event_synchronize(void* ev);     /* host waits until the work before ev is done */
/* extra streams for concurrent work (e.g. a communication stream);
 * hpa_stream_wait_event: the CURRENT stream waits for `ev` (recorded on any
 * stream).  Inside a capture, fork/join through events pulls the other
 * stream into the same graph as parallel branches. */
void* hpa_stream_create(void);
int   hpa_stream_destroy(void* stream);
int   hpa_stream_wait_event(void* ev);
/* a dependency through a device word (round 6): write_value -- the current
 * stream sets *flag = value once its earlier work is done; wait_value -- the
 * current stream waits until *flag >= value.  The decode gather's
 * compute -> comm hand-off uses it: a pending event wait on another stream
 * slows the decode stream's kernels ~25 us per step, a pending wait-value
 * 5-9 us (profiles/r6/recv_coresidency.txt). */
int   hpa_stream_value_ops(void);  /* 1 if the device supports them (else use events) */
int   hpa_stream_write_value32(unsigned* flag, unsigned value);
int   hpa_stream_wait_value32(unsigned* flag, unsigned value);
const char* hpa_last_error(void);
/* build flags of this library: bit 0 = an A/B build (-DHPA_AB: the layer
 * forms measured slower -- the full persistent layer, the wide-unit chains --
 * and the measurement env knobs HPA_LAYER_SPLITS, HPA_GEMM_RING,
 * HPA_LOGITS_FORM, HPA_BF16_ARES; the product library has none of them) */
int hpa_build_flags(void);
/* hipGraph capture of everything enqueued on the current stream between
 * begin and end (the decode step: 5 launches per layer); replay with
 * hpa_graph_launch.  Kernel arguments are frozen at capture, so per-step
 * state (tokens, positions, block tables) must live in device memory. */
int   hpa_graph_begin(void);
void* hpa_graph_end(void);               /* instantiated executable graph, NULL on failure */
int   hpa_graph_launch(void* graph_exec);
int   hpa_graph_destroy(void* graph_exec);
/* waves per (sequence, head) workgroup of every decode attention launch of
 * the process: 1, 2, 4, 8 (an override for timing tools); 0 (default): the
 * caller's choice (the engine's hpa_attn_pick_waves, else 4) */
int   hpa_set_attention_waves(int nw);
int   hpa_attention_waves(void);        /* the override in force (0: none) */
int   hpa_device_info(char* name, int name_len, int* num_cus, size_t* total_mem);

/* ---------------- paged KV pool (fast layout) ----------------
 * One allocation per device: pool[layer][page][kv][head][tile], tile =
 * page_size x head_size elements.  K tiles are stored as
 * [head_size/4][page_size][4] (so one wave64 instruction reads 4-byte x 4
 * columns of 64 consecutive tokens = 128..512 contiguous bytes per page, the
 * lane-per-token QK^T layout); V tiles are token-major [page_size][head_size]
 * (one 256-byte row per token-head, the lane-per-dimension PV layout).
 * bf16 pools (HPA_BF16, BASELINE config 5; storage only, all arithmetic
 * fp32): K tiles [head_size/8][page_size][8] (one 16-byte chunk per
 * lane-per-token load), V tiles [page_size][head_size] (128-byte rows);
 * values are rounded to nearest-even when appended.  Page size multiple of 8.
 * fp8 pools (HPA_FP8; storage only, lossy -- 3 mantissa bits -- all
 * arithmetic fp32): one byte per element in the OCP e4m3fn encoding (bias 7,
 * max 448, no infinities, NaN = 0x7f / 0xff, subnormals down to 2^-9: the
 * encoding of torch.float8_e4m3fn, not the MI300 fnuz form).  K tiles
 * [head_size/16][page_size][16] bytes (one 16-byte chunk per lane-per-token
 * load: a 64-token tile is 4 loads per lane), V tiles [page_size][head_size]
 * bytes (64-byte rows).  Page size 16, 32 or 64.  page_elems / layer_elems
 * stay element counts (for fp8 also the byte counts).
 * One fp32 scale per (layer, K|V, head): `scales`, device memory
 * [num_layers][2][num_heads][2] = (scale, inv), 1.0 / 1.0 after
 * hpa_pool_create; NULL for fp32 and bf16 pools.  A stored value is
 *   code = e4m3fn_rne(clamp(x * inv, -448, 448))
 * (fp32 product; the clamp in fp32 before the convert, so overflow saturates
 * to +-448; NaN stays NaN) and a code stands for decode(code) * scale (fp32
 * product).  Kernels read the scales from device memory at run time, so a
 * captured graph stays valid when they change.  Calibration is the caller's
 * job (per-head max |K|, max |V| of an fp32-pool run, divided by 448).
 * A page id names the same slot in every layer's pool (vLLM-style shared
 * block table), so the block table is [seq][logical page] int32. */
typedef struct HpaKVPool {
    void*  base;          /* device pointer */
    int    num_layers, num_heads, head_size, page_size, num_pages;
    int    dtype;         /* HPA_F32, HPA_BF16 or HPA_FP8 */
    size_t elem_bytes;
    size_t page_elems;    /* elements of one page of one layer (K and V, all heads) */
    size_t layer_elems;   /* num_pages * page_elems */
    size_t bytes;
    int    managed;
    float* scales;        /* fp8 pools: device [num_layers][2][num_heads][2] (scale, inv); else NULL */
} HpaKVPool;
enum { HPA_F32 = 0, HPA_BF16 = 1, HPA_FP8 = 2 };
int  hpa_pool_create(HpaKVPool* pool, int num_layers, int num_heads, int head_size, int page_size,
                     int num_pages, int dtype, int managed);
void hpa_pool_destroy(HpaKVPool* pool);
/* fp8 pools: the per-head scales of K and V, host arrays [num_layers][num_heads]
 * each, every entry finite and > 0 (else nonzero, nothing stored).  Stores
 * (scale, inv = 1.0f / scale), inv computed once here in fp32.  Codes already
 * in the pool keep their bytes and change their meaning: set the scales
 * before anything is appended.  Nonzero on an fp32 / bf16 pool. */
int  hpa_pool_set_scales(const HpaKVPool* pool, const float* host_k_scale, const float* host_v_scale);
/* device address of the K (kv=0) or V (kv=1) tile of (layer, page, head) */
void* hpa_pool_tile(const HpaKVPool* pool, int layer, int page, int kv, int head);
/* host-side layout helpers (tests / compat copies) */
size_t hpa_pool_k_index(const HpaKVPool* pool, int layer, int page, int head, int slot, int d);
size_t hpa_pool_v_index(const HpaKVPool* pool, int layer, int page, int head, int slot, int d);
/* whole pages copied inside the pool, every layer: for i < n the page_elems *
 * elem_bytes contiguous bytes of page src_pages[i] (K and V, all heads) go to
 * page dst_pages[i] in each layer's slab.  Bytes only, whatever the dtype (an
 * fp8 pool's scales are per (layer, head), not per page).  src_pages and
 * dst_pages are HOST arrays of pool slots, 1 <= n <= HPA_COPY_MAX_PAGES; they
 * travel by value in the kernel arguments: ONE asynchronous launch on the
 * current stream, no staging buffer, no sync.  Every slot must be in range,
 * every destination distinct, and no page both a source and a destination;
 * otherwise nonzero and nothing is launched. */
#define HPA_COPY_MAX_PAGES 64
int  hpa_pool_copy_pages(const HpaKVPool* pool, const int* src_pages, const int* dst_pages, int n);
/* whole pages between the pool and ONE contiguous buffer, every layer (the data
 * path of gpt2_decode_park / gpt2_decode_unpark).  The buffer holds page i of
 * layer l at byte hpa_park_offset(pool, n_pages, l, i) = (l * n_pages + i) *
 * page_bytes, page_bytes = page_elems * elem_bytes, hpa_park_bytes(pool,
 * n_pages) = num_layers * n_pages * page_bytes in all (both pure host
 * arithmetic: they read the pool's shape only): the layout does not depend on
 * where the pages sat in the pool.  Bytes only, whatever the dtype.
 * gather: page pages[i] of every layer -> the buffer; scatter: the buffer ->
 * page pages[i] of every layer.  pages is a HOST array of pool slots, n_pages
 * >= 1 without an upper bound; dst / src is 16-byte aligned memory a kernel may
 * dereference over all hpa_park_bytes (device memory, or pinned host memory:
 * hpa_is_device_accessible).  ceil(n_pages / HPA_PARK_MAX_PAGES) asynchronous
 * launches on the current stream, each over every layer with its page ids by
 * value in the kernel arguments: no staging table, no sync, no allocation.  A
 * slot out of range, a slot listed twice in a scatter, or an inaccessible
 * buffer: nonzero and nothing is launched. */
#define HPA_PARK_MAX_PAGES 64   /* page ids per launch, by value in the kernel arguments */
size_t hpa_park_bytes(const HpaKVPool* pool, int n_pages);
size_t hpa_park_offset(const HpaKVPool* pool, int n_pages, int layer, int i);
int  hpa_pool_gather_pages(const HpaKVPool* pool, const int* pages, int n_pages, void* dst);
int  hpa_pool_scatter_pages(const HpaKVPool* pool, const int* pages, int n_pages, const void* src);
/* the pool side of the two kernels as non-temporal accesses (a measurement
 * knob of tools/park_scan.py): bit 0 the gather's loads, bit 1 the scatter's
 * stores.  3 (default): both (profiles/r18/park.txt: the loads a measured gain, the
 * stores a wash) */
int  hpa_park_set_nontemporal(int mask);
int  hpa_park_nontemporal(void);

/* ---------------- decode-step kernels (fp32) ----------------
 * B = sequences in the batch, C = channels, NH heads of head_size 64.
 * pos[b] = absolute position of the token decoded this step (== tokens
 * already cached for b); the token's K/V go to slot pos[b] and attention
 * covers positions 0..pos[b]. */

/* paged decode attention (attention_paged paged_infer.c:163-240 for one
 * query row per sequence at absolute position pos[b]): block-table gather of
 * K/V pages -> q.k^T -> online softmax -> PV.  q, out: [B][C]. */
int hpa_paged_attention_decode(const float* q, const HpaKVPool* pool, int layer,
                               const int* block_table, int bt_stride, const int* pos, float* out,
                               int B);

/* split-context (flash-decoding) form: each (sequence, head)'s context is cut
 * into `splits` (1..HPA_ATTN_MAX_SPLITS) ranges of 64-token tiles, one
 * workgroup each; the last range to finish merges the ranges' (max, sum,
 * acc) in range order (so the result does not depend on timing) and writes
 * out[b] -- row-major [B][C] or, out_frag != 0, the frag layout.  ws:
 * hpa_attn_ws_bytes(B, NH, splits) bytes of device memory whose counter part
 * is zero before the first launch (hpa_memset_async the whole buffer once;
 * every launch leaves it zero).  splits = 1 is the single-pass kernel above
 * (ws may be NULL).  Within fp32 rounding of the single pass (another
 * summation grouping), bit-identical across launches for a given splits. */
#define HPA_ATTN_MAX_SPLITS 16
size_t hpa_attn_ws_bytes(int B, int num_heads, int splits);
/* the engine's choice by shape only (num_cus <= 0: 256): ranges while B*NH*S
 * stays within one workgroup per CU, 2 between one and two per CU, else 1 */
int hpa_attn_pick_splits(int B, int num_heads, int max_ctx, int num_cus);
/* the same with the waves per workgroup (0: 4; 1, 2, 4 or 8) -- the engine
 * passes hpa_attn_pick_waves of its (global) batch */
int hpa_paged_attention_decode_split_w(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                       int bt_stride, const int* pos, float* out, int B, int splits, void* ws,
                                       int out_frag, int waves);
/* 8 when the B*num_heads*splits workgroups fit one per CU, else 4 */
int hpa_attn_pick_waves(int B, int num_heads, int splits, int num_cus);
int hpa_paged_attention_decode_split(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                     int bt_stride, const int* pos, float* out, int B, int splits, void* ws,
                                     int out_frag);

/* ---------------- shared-prefix decode attention (hpa_attn_shared.hip) ----
 * out[b] is hpa_paged_attention_decode's: row b over keys 0 .. pos[b], the
 * -10000 floor and the zero row included.  The device tables only decide which
 * workgroup streams which tiles: a unit is up to HPA_SHARED_MAX_ROWS sequences
 * that hold the SAME pages for tokens [0, 64 * unit_tiles) and have at least
 * that many cached (gpt2_attn_shared_plan, paged_infer.h, builds them).
 *   unit_members [max_units][HPA_SHARED_MAX_ROWS]  sequence indices, -1 padded
 *   unit_tiles   [max_units]                       64-token tiles, 0 = unused
 *   seq_skip     [B]                               the tiles b's unit streams, else 0
 * Two launches on the current stream: the prefix launch, grid max_units x
 * num_heads x prefix_splits, streams each unit's tiles once for all its
 * members' rows (page ids from the first member's table row, no key masked)
 * and writes the unnormalised (m, l, acc) of every (member, head, split) as a
 * 68-float record into ws; the suffix launch, one workgroup per (sequence,
 * head), is the decode kernel from tile seq_skip[b] on, whose final fold takes
 * in b's records in split order ahead of its wave states.  No in-launch
 * hand-off: the records cross the kernel boundary.  A launch repeats bit for
 * bit; with every unit_tiles and seq_skip 0 (or max_units 0) the bits are
 * hpa_paged_attention_decode_split_w(splits = 1) at the same waves, and so is
 * every row outside the units.  ws: hpa_attn_shared_ws_bytes, 16-byte aligned,
 * needs no zeroing.  waves: the suffix workgroup's (0: 4; 1, 2, 4, 8); the
 * prefix workgroup has 8 waves when that is 8, else 4.
 * Nonzero, nothing launched: a pool that is not fp32, head size != 64, a page
 * size other than 8 / 16 / 32 / 64, prefix_splits outside 1 ..
 * HPA_ATTN_MAX_SPLITS, a null or misaligned ws with max_units > 0. */
#define HPA_SHARED_MAX_ROWS 8
size_t hpa_attn_shared_ws_bytes(int B, int num_heads, int prefix_splits);
/* the engine's prefix_splits, pure, by shape only (num_cus <= 0: 256): the
 * smallest power of two at which units * num_heads * splits reaches two
 * workgroups per CU, capped so that a range keeps about three of the largest
 * unit's max_tiles tiles */
int hpa_attn_shared_pick_splits(int units, int num_heads, int max_tiles, int num_cus);
int hpa_paged_attention_decode_shared(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                      int bt_stride, const int* pos, float* out, int B, const int* unit_members,
                                      const int* unit_tiles, int max_units, const int* seq_skip, int prefix_splits,
                                      void* ws, int out_frag, int waves);
/* synthetic K/V fill of positions [0, ctx) for every sequence with U(-1,1)
 * from a counter-based hash (attention microbench / bench synthetic prefill) */
int hpa_pool_fill_random(const HpaKVPool* pool, const int* block_table, int bt_stride, int B,
                         int ctx, uint64_t seed);
/* the same for sequences seq_offset .. seq_offset+B-1 of a larger batch (a
 * shard fills exactly the rows the unsharded batch would get) */
int hpa_pool_fill_random_ex(const HpaKVPool* pool, const int* block_table, int bt_stride, int B,
                            int ctx, uint64_t seed, int seq_offset);

/* ---------------- fused decode-layer GEMMs (the engine's path) ----------------
 * "frag" layout: a [rows][K] fp32 matrix with rows padded to a multiple of 16
 * stored so that the v_mfma_f32_16x16x4_f32 operand fragment of (16-row
 * block, 16-deep k-step) is 1 KiB contiguous: element (m,k) at
 * ((m/16 * K/16 + k/16) * 64 + m%16 + 16*((k%16)/4)) * 4 + k%4.  Weights are
 * packed once at load; activations that feed a GEMM are written in it. */
size_t hpa_frag_elems(int rows, int K);           /* padded element count */
int hpa_pack_frag(const float* src, int rows, int K, int ld, float* dst); /* device -> device */
int hpa_unpack_frag(const float* src, int rows, int K, float* dst, int ld);
/* bf16 frag layout ([rows][K], rows padded to 16, K % 32 == 0): the
 * v_mfma_f32_16x16x32_bf16 operand fragment of (16-row block, 32-deep k-step s)
 * is 1 KiB contiguous; lane l = (m % 16) + 16*g holds k = 32s + 4g + {0..3} then
 * k = 32s + 16 + 4g + {0..3} (the two float4 the same lane reads from the fp32
 * frag layout at k16-steps 2s, 2s+1).  Element (m, k) at
 * ((m/16 * K/32 + k/32) * 64 + m%16 + 16*((k%16)/4)) * 8 + k%4 + 4*((k%32)/16).
 * Values are fp32 rounded to nearest even (hpa_pack_frag_bf16, device -> device). */
size_t hpa_frag_bf16_elems(int rows, int K);      /* padded element count (2 bytes each) */
int hpa_pack_frag_bf16(const float* src, int rows, int K, int ld, void* dst);

/* per-row LayerNorm statistics travel between kernels as partial sums
 * (sum x, sum x^2) over 16-column tiles: stats[tile][Mp][2]; a consumer sums
 * the `ntiles` partials of a row in order: mean = S1/C, var = S2/C - mean^2,
 * rstd = 1/sqrtf(var + 1e-5) (layernorm_forward, paged_infer.c:49-89, in its
 * one-pass form) and applies (x - mean) * rstd * w + b to its A fragments. */
enum { HPA_FEPI_QKV = 0, HPA_FEPI_RESID = 1, HPA_FEPI_GELU = 2, HPA_FEPI_LOGITS = 3, HPA_FEPI_SCORE = 4 };
typedef struct {
    /* A = x (frag layout, M rows, K cols), optionally LayerNorm'ed on the fly */
    const float* x;
    int M, K;
    const float* ln_stats; /* NULL: no LN */
    int ln_ntiles;
    const float* ln_w;
    const float* ln_b;
    /* B = W^T, W (frag layout, N rows of K) */
    const float* w;
    int N;
    const float* bias;    /* [N] or NULL */
    int epilogue;         /* HPA_FEPI_* */
    /* QKV: out = q [M][C] row-major; K/V rows appended to pool pages at pos[m] */
    /* RESID: out = res_in + acc + bias (frag layout [M][N]); stats_out[N/16][Mp][2]
       (NULL: no statistics -- the consumer folds its LN and sums its own) */
    /* GELU: out = gelu(acc + bias) (frag layout [M][N]) */
    /* LOGITS: out = acc [M][N] row-major (ld = N); part_out[N/16 tiles][Mp][2] = (max, argmax) */
    /* SCORE: the LOGITS arithmetic with a log-softmax epilogue: no out (may be NULL), the logits
       never reach memory; score_part[N/16 tiles][Mp][4] row partials (below) */
    float* out;
    const float* res_in;
    float* stats_out;
    float* part_out;
    const HpaKVPool* pool;
    int layer;
    const int* block_table;
    int bt_stride;
    const int* pos;
    int waves;            /* waves per workgroup sharing the K range: 4, 8 or 16; 0 = by shape.
                             Variant 4 on the resident logits kernel: 16 = its 16-wave
                             K-split form, 12 = its ring form, else by M (the two sum a
                             row's K in different orders: give sharded callers the
                             global batch's form) */
    int row_blocks;       /* 16-row blocks per workgroup: 1, 2 or 4; 0 = by shape */
    int variant;          /* 0 = by shape; 1 = looped (two trips in flight);
                             2 = one-shot (every operand load issued up front; one
                             row block; (waves, K/16) in {(4,48),(8,48),(16,48),(8,192),(16,192),(10,100)});
                             3 = loader / MFMA-wave ring (hpa_gemm_ring.hip): <= 64 padded rows,
                             LN folded (ln_fold_c1) or absent, QKV / GELU / RESID; one
                             12-wave workgroup per 32 columns and K part; waves = K parts
                             (0/1 = none; 2..4 need sk_slab / sk_count sized by
                             hpa_gemm_ring_workspace: the last part of a column pair sums
                             the parts in part order); row_blocks / col_tiles ignored;
                             4 = LOGITS only: activation-resident persistent kernel
                             (K = 768, rows <= 64; 16 waves); else stream-K (6) when
                             sk_slab / sk_count are given and rows <= 64; else as 1;
                             5 = bf16 weights only: A-resident kernel (col_tiles = rounds,
                             K <= 3200);
                             6 = stream-K (hpa_gemm_sk.hip; M <= 64, fp32 weights): one
                             8-wave workgroup per CU walks an equal contiguous share of
                             the (32-column super-tile, k16) steps, all M rows at once;
                             tiles split between workgroups are summed in workgroup
                             order by the last to arrive (sk_slab / sk_count).  LN
                             folded (ln_fold_c1) or applied on load (K <= 2048) */
    int col_tiles;        /* 16-column tiles per workgroup: 1; 2 (waves 4/8, row_blocks
                             2/4); 4 (waves 4, row_blocks 4); 0 = by shape.  A hint:
                             where M's row blocks or the waves cannot carry it, 1 */
    const int* row_seq;   /* QKV: block-table row of each GEMM row (NULL = the row
                             itself; prefill rows b*T+t -> b); LOGITS (looped and
                             bf16 kernels): the output row of each GEMM row
                             (gpt2_forward's per-position logits, written in place) */
    const float* ln_fold_c1; /* non-NULL: the LayerNorm is folded into w (packed by
                             hpa_ln_fold_pack: w = W*ln_w per column k, bias = c2):
                             A is x as it stands, and the epilogue applies
                             out[n] = rstd*(acc[n] - mean*c1[n]) + bias[n] with the
                             row statistics (one-pass) summed from the A fragments
                             the workgroup already holds (K = the LN width).  No LN
                             prologue and no statistics loads; ln_stats, ln_w and
                             ln_b are not read. */
    float* sk_slab;       /* variant 6: hpa_gemm_sk_workspace floats */
    int* sk_count;        /* variant 6: per-super-tile counters, zero before the first launch
                             (every launch leaves them zero) */
    int w_dtype;          /* HPA_F32 (0): w is fp32 frag layout.  HPA_BF16: w points at bf16
                             weights in the bf16 frag layout (hpa_pack_frag_bf16), K % 32 == 0;
                             A is rounded to bf16 (RNE) after the LayerNorm, products are
                             summed in fp32 on v_mfma_f32_16x16x32_bf16 (variant 0, 1
                             or 5; ln_fold_c1 must be NULL); waves 4/8. */
    /* LOGITS on the activation-resident kernel (variant 4, fp32) only: non-NULL
     * pick_next makes the launch's last workgroup to finish (an arrival ticket on
     * pick_count: one int, zero before the first launch, left zero) reduce the
     * argmax partials as hpa_argmax_final(part_out, ..., pick_next, pick_tokens,
     * pick_pos, NULL) would: next[m] = the lowest column of row m's maximum;
     * pick_tokens (nullable) gets it too, pick_pos (nullable) += 1.  Saves the
     * argmax launch. */
    int* pick_next;
    int* pick_tokens;
    int* pick_pos;
    int* pick_count;
    /* SCORE (looped fp32 kernel: variant 0 / 1; bf16 weights: variant 0 / 1 / 5; any other
     * variant is refused).  score_target: device [M], the column whose logit each row
     * reports, -1 (or a NULL array) = none.  score_part: device, hpa_score_workspace(N,
     * Mp) floats, 16-byte aligned; per (16-column tile t, row m) one float4 at
     * [(t * Mp + m) * 4]:
     *   .x  m_t = the maximum of the tile's columns < N
     *   .y  sum over those columns of expf(v - m_t), added in column order
     *   .z  the target's logit when the target column lies in the tile, else -inf
     *   .w  the bits of the tile's first-maximum column (lowest column wins, as LOGITS)
     * Rows M <= m < Mp get (-inf, 0, -inf, 16 t): no NaN.  hpa_score_final combines them. */
    const int* score_target;
    float* score_part;
} HpaFusedGemm;
/* LayerNorm folding for hpa_gemm_fused (layernorm_forward :49-89 followed by
 * matmul_forward :92-114, restated): for W [N][K] row-major (device), writes
 * dst_frag = frag-packed W[n][k]*ln_w[k], c1[n] = sum_k of those products and
 * c2[n] = sum_k ln_b[k]*W[n][k] + bias[n] (bias may be NULL); sums in double,
 * rounded once.  Then sum_k LN(x)_k W[n][k] + bias[n] =
 * rstd*(sum_k x_k W'[n][k] - mean*c1[n]) + c2[n]. */
int hpa_ln_fold_pack(const float* W, int N, int K, const float* ln_w, const float* ln_b, const float* bias,
                     float* dst_frag, float* c1, float* c2);
int hpa_gemm_fused(const HpaFusedGemm* g);
/* variant 3 K-split workspace for an (N) GEMM in `parts` K parts: slab
 * floats and counters (zero before the first launch; every launch leaves them
 * zero); nonzero on bad arguments */
int hpa_gemm_ring_workspace(int N, int parts, size_t* slab_floats, size_t* counters);
/* variant 6 workspace: slab floats and counters for an (N) GEMM on this
 * device's CU count (enough for any K and M <= 64) */
int hpa_gemm_sk_workspace(int N, size_t* slab_floats, size_t* counters);
/* argmax partials per row a LOGITS launch of g writes into part_out (the
 * `ntiles` of hpa_argmax_final): N/16 tiles, or one per workgroup of the
 * activation-resident kernel (variant 4) on the current stream; -1 if g is
 * not a valid LOGITS descriptor */
int hpa_logits_partials(const HpaFusedGemm* g);
/* the kernel a variant-4 fp32 LOGITS GEMM of this shape runs (LN applied):
 * 4 = activation-resident, 6 = stream-K (when given its workspace), 1 =
 * looped; -1 on a bad shape.  The engine allocates the stream-K workspace
 * exactly when this says 6. */
int hpa_logits_kernel(int M, int N, int K);
/* the launch shape hpa_gemm_fused picks when waves / row_blocks / col_tiles
 * are 0: out3 = {waves, row_blocks, col_tiles} */
void hpa_fused_pick(int M, int N, int K, int* out3);
/* the launch shape of a bf16-weight GEMM (w_dtype = HPA_BF16) when waves /
 * row_blocks / col_tiles are 0 */
void hpa_fused_pick_bf16(int M, int N, int K, int* out3);
/* bf16 weights, A-resident kernel (variant 5: the workgroup's rows of A
 * LayerNorm'ed and rounded into LDS once, waves walking waves*rounds column
 * tiles over the whole K; col_tiles = rounds for this variant):
 * out3 = {waves, row_blocks, rounds}; returns 1 where variant 0 uses it */
int hpa_fused_pick_bf16_ares(int M, int N, int K, int* out3);
int hpa_fused_pick_waves(int M, int N, int K);
/* ---------------- persistent decode layer (hpa_layer.hip and the form files behind it) ----------------
 * The decode step's layer loop (reference gpt2_forward, paged_infer.c:659-722)
 * as ONE launch per layer l instead of five:
 *   attention(l) -> attproj(l) -> fc(l) -> fcproj(l) -> qkv(l+1)
 * or, chain_only, the decode attention as its own launch before and one
 * launch of attproj(l) -> fc(l) -> fcproj(l) -> qkv(l+1) (the engine's
 * default form: measured faster at every batch, profiles/r3/pl_ab.txt).
 * One 12-wave workgroup per CU (grid = CU count, residency checked with the
 * occupancy API), split into three 4-wave slots; every phase deals its units
 * (a 16x16 output tile over a K range, or an attention unit) one per slot.
 * Each slot loads its next phase's weight fragments into registers BEFORE
 * that phase's wait, so the weight stream overlaps the hand-off.  Hand-offs
 * inside the launch: write-through (sc1) stores, drained, one agent-scope
 * arrival per workgroup on a counter sharded 8 ways, polled with sc1 loads
 * (MI355X_MICROARCH.md "Valid forms", row 1).  fcproj is split over K into 4
 * parts and the last part of a tile to draw its ticket adds the parts in part
 * order.  qkv and fc follow the one-shot kernel's summation order (4 waves x
 * K/4, folded in wave order): their rows are bit-identical to the launch path.
 * fp32 frag-packed weights with the LayerNorms folded (hpa_ln_fold_pack);
 * C = 128 or 768 (num_heads 2 or 12), B <= 64, B*num_heads*splits <= 3 x CUs.
 * Every spin is bounded (200 ms): a timeout stores a nonzero code in *err and
 * ends the launch (the outputs are then garbage). */
typedef struct {
    int B, C, num_heads, splits;  /* splits: context ranges of the attention */
    int last;                     /* 1: no qkv(l+1) phase (last layer) */
    int chain_only;               /* 0..6 or 8; the engine's value is DecPlan.chain
                                     (gpt2_decode_layer_plan, paged_infer.h).  0: the full layer,
                                     attention phase first (A/B builds only, like 2..5);
                                     1: no attention phase -- the caller launched the decode
                                     attention (frag output into att) before: the launch is
                                     attproj -> fc -> fcproj -> qkv(l+1); 2..5: the same with wide
                                     units (C = 768), waves per unit of (attproj, fc / fcproj,
                                     qkv): 2 (12, 12, 12) B <= 16; 3 (12, 6, 6) B <= 32;
                                     4 (12, 4, 6) B <= 48; 5 (12, 4, 4) B <= 64; 6: every phase
                                     in units of all 12 waves of a workgroup holding T 16-column
                                     tiles (T by batch, one unit per workgroup, the 12-wave
                                     summation order at every B <= 64), 16-byte epilogues,
                                     waits per row block (C = 768); 8: the chain for
                                     MFMA-bound wide layers (C = 768, 1024, 1280 or 1600: GPT-2 124M to XL): units of
                                     12 waves x up to 7 tiles, weights streamed per tile */
    const HpaKVPool* pool;
    int layer;
    const int* block_table;
    int bt_stride;
    const int* pos;
    const float* q;               /* q of layer l [B][C] row-major (read) */
    float* att;                   /* attention output, frag [Mp][C] */
    float* res;                   /* residual in (frag [Mp][C]); fcproj writes the next */
    float* res2;                  /* res + attproj, frag [Mp][C] */
    float* fch;                   /* gelu(fc), frag [Mp][4C] */
    const float* w_ap;            /* frag-packed attprojw [C][C] */
    const float* b_ap;
    const float* w_fc;            /* LN2-folded fcw [4C][C] */
    const float* fc_c1;
    const float* fc_c2;
    const float* w_fp;            /* frag-packed fcprojw [C][4C] */
    const float* b_fp;
    const float* w_qkv;           /* layer l+1, LN1-folded qkvw [3C][C] (unused when last) */
    const float* qkv_c1;
    const float* qkv_c2;
    float* q_out;                 /* q of layer l+1 [B][C]; its K/V go into layer l+1's pages */
    float* stats_out;             /* last layer: LNf statistics [C/16][Mp][2] of res; else NULL */
    float* rec;                   /* attention split records (hpa_decode_layer_sizes) */
    float* slab;                  /* K-part partial sums */
    int* counters;                /* this layer's counter block, zero before the launch */
    int* err;                     /* this step's: 0, or the code of the first timed-out wait; zeroed
                                     with the counters before every step (the launch's waits bail
                                     out at once when it is set) */
    int* err_sticky;              /* nullable: the first code also lands here, never zeroed by a
                                     step (gpt2_decode_status reads and clears it) */
    int stats_mp;                 /* row stride of stats_out; 0: this launch's Mp */
} HpaLayerArgs;
/* The eligibility predicates and the split pick come in two forms: *_cus
 * takes the CU count as an argument and reads no device (num_cus <= 0: not
 * eligible; the plan function gpt2_decode_layer_plan calls only these); the
 * plain name passes the current device's CU count. */
/* 1 if the persistent layer (chain_only 0..5) applies (C = 128 or 768, shape, CU count), else 0 */
int hpa_decode_layer_eligible_cus(int B, int C, int num_heads, int splits, int num_cus);
int hpa_decode_layer_eligible(int B, int C, int num_heads, int splits);
/* 1 if chain form `form` (HpaLayerArgs.chain_only 6: C = 768; 8: C = 768,
 * 1024, 1280 or 1600) applies to B rows on num_cus CUs, else 0 (any other form: 0) */
int hpa_decode_chain_eligible_cus(int B, int C, int num_heads, int form, int num_cus);
int hpa_decode_chain_eligible(int B, int C, int num_heads, int form);
/* splits the full persistent layer uses by default for this batch (num_cus <= 0: 1) */
int hpa_decode_layer_pick_splits_cus(int B, int num_heads, int max_ctx, int num_cus);
int hpa_decode_layer_pick_splits(int B, int num_heads, int max_ctx);
/* sizes: out[0] = rec floats, out[1] = slab floats, out[2] = counter ints per layer */
int hpa_decode_layer_sizes(int B, int C, int num_heads, int splits, size_t* out3);
int hpa_decode_layer(const HpaLayerArgs* a);
/* the decode step's first launch at GPT-2 124M shapes (C = 768, 12 heads,
 * B <= 64, LN1 folded into w_qkv / qkv_c1 / qkv_c2 of layer 0): the embedding
 * wte[tokens[b]] + wpe[pos[b]] (encoder_forward, paged_infer.c:41-47) into
 * res (frag), layer 0's q into q_out and its K/V into layer 0's pages (chain
 * form 6's qkv phase), and zero_bytes of `zero` (the step's counter block,
 * 16-byte granules) zeroed -- one launch for the embed kernel and the qkv
 * GEMM.  Reads a->B, pool, block_table, bt_stride, pos, res, w_qkv, qkv_c1,
 * qkv_c2, q_out; the layer fields are ignored. */
int hpa_decode_first(const HpaLayerArgs* a, const int* tokens, const float* wte, const float* wpe, void* zero,
                     size_t zero_bytes);
/* ---------------- pipelined halves (hpa_pipe.hip) ----------------
 * The whole layer loop of a decode step (gpt2_forward, paged_infer.c:659-722,
 * every layer l = 0..L-1: attention(l) -> attproj(l) -> fc(l) -> fcproj(l) ->
 * qkv(l+1)) as ONE persistent launch, after the step's first launch
 * (hpa_decode_first: embedding, qkv(0), the counter block zeroed) and before
 * the logits.  The batch is cut into two halves of row blocks; the CUs take
 * fixed roles: `g_cus` CUs run the GEMM chain of one half while the others
 * stream the paged attention of the other half (software pipeline, slot s:
 * attention(s/2, s%2) beside chain((s-1)/2, (s-1)%2)).  The attention is
 * paged_attn_decode_f32's (4 waves per (sequence, head), one context range)
 * and the chain units are chain form 6's (12 waves over K), so a step equals
 * the chain-form step bit for bit.  GPT-2 124M shapes: C = 768, 12 heads,
 * fp32 weights (LN-folded frag packs) and an fp32 pool, 17..64 rows with both
 * halves non-empty.  Bounded spins, error words as hpa_decode_layer. */
typedef struct {
    const float *w_ap, *b_ap;                 /* layer l: attprojw (frag), attprojb */
    const float *w_fc, *fc_c1, *fc_c2;        /* LN2-folded fcw (frag), c1, c2 */
    const float *w_fp, *b_fp;                 /* fcprojw (frag), fcprojb */
    const float *w_qkv, *qkv_c1, *qkv_c2;     /* layer l+1's LN1-folded qkvw (NULL at the last layer) */
} HpaPipeLayer;
typedef struct {
    int B, num_layers;
    const HpaKVPool* pool;        /* fp32 pages; layer l+1's K/V appended by qkv(l+1) */
    const int* block_table;
    int bt_stride;
    const int* pos;
    const HpaPipeLayer* layers;   /* DEVICE array [num_layers] */
    float* q;                     /* q [B][C] row-major: layer 0's from the first launch, rewritten per layer */
    float* att;                   /* frag [Mp][C] */
    float* res;                   /* residual (frag [Mp][C]): the embedding in, the last layer's out */
    float* res2;                  /* frag [Mp][C] */
    float* fch;                   /* frag [Mp][4C] */
    float* slab;                  /* fcproj K-part partials: hpa_decode_pipe_sizes out[0] floats */
    float* stats_out;             /* LNf statistics of the last layer's res [C/16][stats_mp][2] */
    int stats_mp;
    int* counters;                /* [num_layers][layer_ctr_ints], zero before the launch */
    size_t layer_ctr_ints;        /* >= hpa_decode_pipe_sizes out[1] */
    int* err;                     /* as HpaLayerArgs.err / err_sticky */
    int* err_sticky;
    int g_cus;                    /* CUs of the GEMM role (multiple of 8; 0: 64) */
} HpaPipeArgs;
/* 1 if the pipelined-halves launch applies to B rows (C, heads, pool dtype, CU count) */
int hpa_decode_pipe_eligible_cus(int B, int C, int num_heads, int kv_dtype, int num_cus);
int hpa_decode_pipe_eligible(int B, int C, int num_heads, int kv_dtype);
/* out2 = {slab floats, counter ints per layer} */
int hpa_decode_pipe_sizes(int B, size_t* out2);
int hpa_decode_pipe(const HpaPipeArgs* a);
/* diagnostic builds (-DHPA_PIPE_TRACE) only: the per-(layer, half, workgroup)
 * event stamps of the last launch, [2 * layers][256][12] u64 (10-ns ticks);
 * host NULL clears them; returns 1 in the product library */
int hpa_decode_pipe_trace(unsigned long long* host, int layers);
/* ---------------- bf16-weight decode chain (hpa_chain_b16.hip) ----------------
 * The layer's GEMMs on bf16 weights (BASELINE config 5) as ONE persistent
 * launch after the layer's decode-attention launch:
 *   attproj(l) -> fc(l) -> fcproj(l) -> qkv(l+1)
 * (gpt2_forward, paged_infer.c:659-722), in place of four bf16 GEMM launches.
 * C = 768, 12 heads, B = 1..256; one 8-wave workgroup per CU; LayerNorms on
 * the operand path with the row statistics from the consumer's own operand
 * fragments; weights in the bf16 frag layout (hpa_pack_frag_bf16); operands
 * rounded to bf16, fp32 accumulation.  Same hand-off protocol, bounded spins
 * and error words as hpa_decode_layer. */
typedef struct {
    int B, layer, last;           /* last: no qkv(l+1) phase; stats_out then written */
    const HpaKVPool* pool;        /* fp32 or bf16 pages; K/V of layer l+1 appended */
    const int* block_table;
    int bt_stride;
    const int* pos;
    const float* att;             /* attention output of layer l, frag [Mp][C] */
    float* res;                   /* residual in (frag [Mp][C]); fcproj writes the next */
    float* res2;                  /* res + attproj, frag [Mp][C] */
    float* fch;                   /* gelu(fc), bf16 frag layout [Mp][4C] (half the buffer) */
    const void* w_ap;             /* bf16 frag packs: attprojw [C][C], fcw [4C][C], */
    const void* w_fc;             /* fcprojw [C][4C], qkvw of layer l+1 [3C][C] */
    const void* w_fp;
    const void* w_qkv;
    const float *b_ap, *ln2_w, *ln2_b, *b_fc, *b_fp, *ln1_w, *ln1_b, *b_qkv; /* ln1 / b_qkv: layer l+1 */
    float* q_out;                 /* q of layer l+1 [B][C] row-major */
    float* stats_out;             /* last layer: LNf statistics [C/16][stats_mp][2] of res; else NULL */
    int stats_mp;                 /* 0: ceil(B/16)*16 */
    float* slab;                  /* fcproj K-part partials (hpa_decode_chain_b16_sizes out[0] floats) */
    int* counters;                /* this layer's counter block (out[1] ints), zero before the launch */
    int* err;                     /* as HpaLayerArgs.err / err_sticky */
    int* err_sticky;
} HpaChainB16Args;
/* 1 if the bf16 chain applies (C = 768, 12 heads, 1..256 rows, a unit per workgroup), else 0 */
int hpa_decode_chain_b16_eligible_cus(int B, int C, int num_heads, int num_cus);
int hpa_decode_chain_b16_eligible(int B, int C, int num_heads);
/* out2 = {slab floats, counter ints per layer} */
int hpa_decode_chain_b16_sizes(int B, size_t* out2);
int hpa_decode_chain_b16(const HpaChainB16Args* a);
/* the step's first launch on this path: the embedding wte[tokens[b]] +
 * wpe[pos[b]] (encoder_forward, paged_infer.c:41-47) into res, layer 0's q
 * and K/V (the chain's qkv phase; w_qkv / b_qkv / ln1_* of layer 0), and
 * zero_bytes of `zero` (the step's counter block) zeroed -- one launch for
 * the embed kernel and the qkv(0) GEMM.  Reads B, pool, block_table,
 * bt_stride, pos, res, w_qkv, b_qkv, ln1_w, ln1_b, q_out. */
int hpa_decode_chain_b16_first(const HpaChainB16Args* a, const int* tokens, const float* wte, const float* wpe,
                               void* zero, size_t zero_bytes);
/* diagnostic builds (-DHPA_LAYER_TRACE) only, else returns 1: the bf16
 * chain's per-(layer, workgroup) event stamps, as hpa_decode_layer_trace */
int hpa_decode_chain_b16_trace(unsigned long long* host, int layers);
/* diagnostic builds (-DHPA_LAYER_TRACE) only, else returns 1: per-(layer,
 * workgroup) event stamps [layers][256][16] of the last launches (10 ns
 * ticks); host = NULL clears them */
int hpa_decode_layer_trace(unsigned long long* host, int layers);
/* diagnostic builds only, else returns 1: chain form 8's fc phase of layer 5,
 * per wave ([256][12][16] u64 s_memtime: A loads issued, each half-tile's
 * MFMAs issued, loop done); host = NULL clears them */
int hpa_decode_cx_wave_trace(unsigned long long* host);
/* diagnostic builds (-DHPA_RG_TRACE) only, else returns 1: the ring logits
 * kernel's per-workgroup stamps of the last launch: [2][256][24] u64, s_memrealtime
 * (10 ns ticks) then s_memtime (shader clock) */
int hpa_logits_trace(unsigned long long* host);
/* residual = wte[tok] + wpe[pos] in frag layout [Mp][C], stats (1 tile) */
int hpa_embed_frag(const int* tokens, const int* pos, const float* wte, const float* wpe,
                   float* res_frag, float* stats, int B, int C);
/* the same, also zeroing zero[0 .. zero_bytes) (16-byte granules): the
 * decode step's hand-off counters without a memset node of their own */
int hpa_embed_frag_zero(const int* tokens, const int* pos, const float* wte, const float* wpe,
                        float* res_frag, float* stats, int B, int C, void* zero, size_t zero_bytes);
/* greedy id from the logits GEMM's per-tile (max, argmax) partials:
 * lowest index wins ties; next[b], tokens[b] = next[b], pos[b] += 1.
 * active (nullable, [B]): rows with active[b] <= 0 are left untouched */
int hpa_argmax_final(const float* part, int ntiles, int Mp, int B, int* next, int* tokens, int* pos,
                     const int* active);
/* ---------------- log-probabilities (hpa_score.hip) ----------------
 * floats in the SCORE partial buffer of an (N)-column GEMM over chunk_rows rows
 * (a positive multiple of 16): ceil(N/16) * chunk_rows * 4.  Host arithmetic
 * only; nonzero on bad arguments. */
int hpa_score_workspace(int N, int chunk_rows, size_t* floats);
/* combines the SCORE partials of rows 0..M-1 (part[ntiles][Mp][4]; rows up to
 * Mp are read, as the SCORE GEMM writes them), one workgroup per four rows, in
 * a fixed order (a launch repeats bit for bit): the row maximum Mx over the
 * tiles, S = sum_t s_t * exp(m_t - Mx) in double (each thread its tiles in
 * increasing order under a running maximum, then a fixed tree), and
 *   lse[m]         = Mx + log S
 *   logprob[m]     = target logit - lse, 0.0f where the row has no target
 *   top_id[m]      = the lowest column of the row's maximum
 *   top_logprob[m] = Mx - lse
 * Any of the four outputs may be NULL. */
int hpa_score_final(const float* part, int ntiles, int Mp, int M, float* logprob, float* lse, int* top_id,
                    float* top_logprob);
/* logprob[b] = logits[b][ids[b]] - logsumexp(logits[b]) for logits [B][V]
 * row-major (the raw distribution: temperature 1, no filter), one workgroup
 * per row, sums in double in a fixed order.  active as hpa_argmax_final: rows
 * with active[b] <= 0 are left untouched.  An id outside [0, V) gives 0. */
int hpa_logprob_rows(const float* logits, int B, int V, const int* ids, const int* active, float* logprob);
/* ---------------- top log-probabilities (hpa_top.hip) ----------------
 * The k best columns of every row of logits [rows][V] (row stride V, rows
 * 4-byte aligned, finite values) and their log-probabilities.  Entry j of a
 * row is its j-th element under: logit descending as a float comparison (-0.0
 * and +0.0 tie), equal logits by ascending column; entry 0 is hpa_argmax_final's
 * pick.  top_lps[r][j] = (float)((double)x[id] - lse_r), lse_r the row's
 * log-sum-exp summed in double in a fixed order (a launch repeats bit for bit;
 * within 4e-6 + 2^-22 max(|lse|, |x[id]|) of the float64 log-softmax).
 *   active    nullable: rows with active[r] <= 0 are left untouched
 *   targets   nullable: per row a column in [0, V) or -1
 *   target_lp nullable with targets: [rows], 0.0 where target == -1
 *   lse       nullable: [rows]
 * Nonzero and nothing launched: k < 1, k > HPA_TOP_LOGPROBS_MAX, k > V, a null
 * required pointer, rows <= 0; also V > 262144 (a row is cut into at most 256
 * slices of 1024 columns).  Two launches (one wave per slice of a row: its k
 * candidates and its (max, sum exp); then one workgroup per row that merges
 * the slices) through a workspace:
 * hpa_top_logprobs keeps one of its own, grown on demand (a growth waits for
 * the stream and cannot happen while a graph is captured);
 * hpa_top_logprobs_ws takes the caller's, 8-byte aligned, of at least
 * hpa_top_logprobs_workspace bytes (enough for every launch of at most that
 * many rows and that k), and the slice count (0: hpa_top_logprobs_slices; any
 * other count needs rows * slices * (12 + 8 k) bytes and gives the same ids). */
#define HPA_TOP_LOGPROBS_MAX 20
int hpa_top_logprobs(const float* logits, int rows, int V, int k, const int* active, const int* targets, int* top_ids,
                     float* top_lps, float* target_lp, float* lse);
int hpa_top_logprobs_workspace(int rows, int V, int k, size_t* bytes);
int hpa_top_logprobs_ws(const float* logits, int rows, int V, int k, const int* active, const int* targets,
                        int* top_ids, float* top_lps, float* target_lp, float* lse, void* ws, size_t ws_bytes,
                        int slices);
/* slices a row is cut into at (rows, V) on num_cus CUs (<= 0: 256); host arithmetic only */
int hpa_top_logprobs_slices(int rows, int V, int num_cus);
/* multinomial draw per row from softmax(logits) with the reference's
 * generator and arithmetic order (softmax_forward :259-286, sample_mult
 * :837-848, random_f32 :826-835), one xorshift state per row advanced on the
 * device; next[b], tokens[b] = next[b], pos[b] += 1 (tokens/pos may be NULL);
 * active as hpa_argmax_final (an inactive row's state does not advance) */
int hpa_sample_final(const float* logits, int B, int V, unsigned long long* state, int* next, int* tokens,
                     int* pos, const int* active);
/* the same draw from the single-lane sequential kernel (the ordered fp32
 * additions as one dependent chain); kept as the measured baseline and as a
 * cross-check of hpa_sample_final's integer-scan formulation */
int hpa_sample_final_serial(const float* logits, int B, int V, unsigned long long* state, int* next, int* tokens,
                            int* pos, const int* active);
/* temperature / top-k / top-p sampling with per-row settings (device arrays
 * [B]: temperature, top_k, top_p).  active, tokens, pos and next as in
 * hpa_sample_final; an inactive row changes nothing, its state included.
 * Per active row b, x = logits[b]:
 *  - coin: the row's xorshift state advances exactly once per call (greedy
 *    rows too), u = (xorshift_u32(state) >> 8) / 16777216.0f;
 *  - temperature[b] == 0: greedy, the argmax of x (lowest index on ties),
 *    n_kept = 1, cut = max x;
 *  - canonical order: tokens by (logit descending, index ascending);
 *  - top-k: k = top_k[b]; 0 or k >= V keeps everything, else the first k
 *    tokens of the canonical order (exact: temperature keeps the order);
 *  - probabilities over the top-k set, T = temperature[b], m = max x:
 *    p_i = exp((x_i - m) / T) / sum_kept exp((x_j - m) / T);
 *  - top-p: P = top_p[b] in (0, 1] keeps the shortest prefix of the canonical
 *    order, inside the top-k set, whose mass is >= P; at least one token;
 *    P = 1 keeps the whole top-k set;
 *  - n_kept[b]: the length of that prefix; cut[b]: the logit of its last
 *    token (both nullable).  The kept set is every token with x > cut plus
 *    the lowest-indexed tokens with x == cut, n_kept in all;
 *  - draw: over the kept tokens in index order (as sample_mult walks them),
 *    renormalised to the kept mass: the first kept index whose running cdf
 *    exceeds u.
 * Bad per-row values cannot index out of range: T < 0 or non-finite counts as
 * 1, k < 0 as 0, P outside (0, 1] as 1.  Sums are fixed-point integers
 * (hpa_sample.hip), so a launch repeated on the same inputs and states
 * returns the same ids. */
int hpa_sample_filtered(const float* logits, int B, int V, const float* temperature, const int* top_k,
                        const float* top_p, unsigned long long* state, int* next, int* tokens, int* pos,
                        const int* active, int* n_kept, float* cut);
/* hpa_sample_filtered with one id per row taken out of the draw: exclude ([B],
 * nullable; -1 or any id outside [0, V): none).  The filter (kept set, n_kept,
 * cut) is decided exactly as above; then exclude[b], if kept, is removed and the
 * draw walks the remaining kept tokens in index order against the total
 * w_total - w_excluded (the same fixed-point masses, the same single coin).  An
 * exclusion that would empty the set is dropped (the excluded id is then the
 * only id left to return); greedy rows ignore it.  n_kept / cut report the
 * filter, not the removal.  With exclude NULL or -1 everywhere every output
 * (ids, states, n_kept, cut) is hpa_sample_filtered's bit for bit;
 * hpa_sample_filtered is this call with NULL. */
int hpa_sample_filtered_ex(const float* logits, int B, int V, const float* temperature, const int* top_k,
                           const float* top_p, unsigned long long* state, int* next, int* tokens, int* pos,
                           const int* active, int* n_kept, float* cut, const int* exclude);
/* The filter alone, for R rows at once, and the mass it gives one id per row:
 * no coin, no state, no draw.  Row r (logits [R][V], rows 4-byte aligned) reads
 * the settings of sequence seq[r] (seq NULL: of sequence r) from the arrays
 * hpa_sample_filtered reads, sanitised the same way, and runs the same passes
 * (one workgroup per row).  Outputs, [R] each:
 *   n_kept, cut  (nullable) hpa_sample_filtered's for that row and settings, bit for bit
 *   w_total      the kept set's fixed-point mass, the total the draw divides by
 *   w_target     the fixed-point mass of target[r] in the draw: 0 when it is
 *                outside the kept set (a tie at the cut that is not kept, an id
 *                below the cut, an id outside [0, V))
 * so p(target) = w_target / w_total, and a coin u = j / 2^24 lies below it iff
 * w_target * 2^24 > w_total * j.  A temperature-0 row reports (w_target,
 * w_total) = (1, 1) when target[r] is the lowest-index argmax and (0, 1)
 * otherwise.  Integer sums: a launch repeats bit for bit. */
int hpa_sample_filtered_prob(const float* logits, int R, int V, const int* seq, const float* temperature,
                             const int* top_k, const float* top_p, const int* target, int* n_kept, float* cut,
                             unsigned long long* w_target, unsigned long long* w_total);
/* The accept / reject walk of speculative sampling with point-mass drafts, one
 * thread per sequence.  Sequence b has len[b] rows (row 0 its pending id, then
 * len[b] - 1 drafts drafts[draft0[b] ..]); w_target / w_total [draft0[b] + i]
 * are hpa_sample_filtered_prob's masses of draft i under the row before it.
 * For i = 0, 1, ..: one coin j = xorshift_u32(state[b]) >> 8; draft i is
 * accepted iff w_target * 2^24 > w_total * j (128-bit integers); the walk stops
 * at the first rejection.  a = the number accepted:
 *   n_accepted[b] = a; cont_row[b] = row0[b] + a; pos[b] = start[b] + a;
 *   exclude[b] = the rejected draft, -1 when every draft was accepted.
 * state[b] has then advanced once per examined draft (the pick that follows
 * advances it once more).  len[b] == 0: n_accepted = cont_row = exclude = -1,
 * state and pos untouched. */
int hpa_spec_accept(const unsigned long long* w_target, const unsigned long long* w_total, const int* drafts,
                    const int* draft0, const int* start, const int* row0, const int* len, int B,
                    unsigned long long* state, int* n_accepted, int* cont_row, int* exclude, int* pos);
/* ---- sampled tree speculation: the list forms (HPA_VERIFY_MAX_ROWS - 1 = 7
 * ids a row at the most) ----
 * hpa_sample_filtered_prob with a list of ids per row: targets [R][7], of which
 * the first n_targets[r] (clamped to [0, 7]) count.  The row is read once
 * whatever the list's length (one tie-rank counter per id); the kept total,
 * n_kept and cut are computed once.  Entry i's mass goes to w_target[dst[r][i]]
 * and the row's total to w_total[dst[r][i]] (dst [R][7]: indices into arrays
 * the caller packs as it likes, hpa_spec_tree_accept's by draft; a negative
 * index writes nothing).  Every (mass, total) pair, n_kept[r] and cut[r]
 * (nullable, [R]) are what hpa_sample_filtered_prob reports for that (row, id),
 * bit for bit: an id outside [0, V) has mass 0, duplicates each get their mass,
 * a temperature-0 row gives (1, 1) to the lowest-index argmax and (0, 1) to
 * anything else.  One workgroup per row. */
int hpa_sample_filtered_prob_multi(const float* logits, int R, int V, const int* seq, const float* temperature,
                                   const int* top_k, const float* top_p, const int* targets, const int* n_targets,
                                   const int* dst, int* n_kept, float* cut, unsigned long long* w_target,
                                   unsigned long long* w_total);
/* hpa_sample_filtered_ex with a list of ids per row taken out of the draw:
 * exclude [B][7], of which the first n_exclude[b] (clamped to [0, 7]) count.
 * Each listed id that is in the kept set loses its mass from the draw and from
 * the total; ids outside [0, V), ids outside the kept set and repeats remove
 * nothing.  If the removals would leave nothing, all of them are dropped (the
 * plain draw).  Greedy rows ignore the list.  One coin; n_kept / cut report the
 * filter, not the removal.  With n_exclude[b] <= 1 every output is
 * hpa_sample_filtered_ex's for that id (or -1) bit for bit. */
int hpa_sample_filtered_exn(const float* logits, int B, int V, const float* temperature, const int* top_k,
                            const float* top_p, unsigned long long* state, int* next, int* tokens, int* pos,
                            const int* active, int* n_kept, float* cut, const int* exclude, const int* n_exclude);
/* The accept walk of sampled tree speculation, one thread per sequence.
 * Sequence b's len[b] rows are the nodes of hpa_verify_tree_rows (node 0 the
 * pending id, draft j = node j + 1 under parents[draft0[b] + j], clamped into
 * [0, j]); w_target / w_total [draft0[b] + j]: draft j's fixed-point mass at
 * its parent's row and that row's kept total (hpa_sample_filtered_prob_multi,
 * the same total for all children of one node).  From cur = node 0:
 *   rem = the total of cur's row; the children c of cur in ascending node
 *   index, one coin j = xorshift_u32(state[b]) >> 8 each: c is accepted iff
 *   w_c * 2^24 > rem * j (128-bit integers) -- then cur = c and the walk
 *   starts over there; else rem -= w_c (a rejected child has w_c < rem) and
 *   the next child is examined.  The walk ends at a leaf or when every child
 *   of cur was rejected.
 * Outputs: n_accepted[b] = a = depth(cur); path[b * HPA_VERIFY_MAX_ROWS + i],
 * i < a: the accepted nodes, strictly increasing; cont_row[b] = row0[b] + cur;
 * pos[b] = start[b] + a (as hpa_verify_tree_accept); exclude [B][7] / n_exclude
 * [B]: the tokens of cur's rejected children in child order (-1 beyond), which
 * hpa_sample_filtered_exn takes out of the sequence's own draw.  state[b]
 * advances once per examined child.  len[b] == 0: n_accepted = cont_row = -1,
 * n_exclude = 0, exclude = -1; state, pos and path untouched. */
int hpa_spec_tree_accept(const unsigned long long* w_target, const unsigned long long* w_total, const int* drafts,
                         const int* parents, const int* draft0, const int* start, const int* row0, const int* len, int B,
                         unsigned long long* state, int* n_accepted, int* path, int* cont_row, int* exclude,
                         int* n_exclude, int* pos);
/* ---------------- logit processors (hpa_process.hip) ----------------
 * Repetition, presence and frequency penalties and a sparse logit bias, per
 * row, from the raw logits [B][V] and a dense count table counts [B][V]
 * (uint16, 4-byte aligned base).  For an active row b and column t, x = the raw
 * logit, c = counts[b][t], in fp32, every step rounded on its own, in this order:
 *     if c > 0:  x = x > 0 ? x / repetition[b] : x * repetition[b]
 *     x = x - frequency[b] * (float)c - (c > 0 ? presence[b] : 0)
 *     if t is in b's bias list:  x = x + its value        (finite, or -inf: a ban)
 * With repetition 1, frequency = presence = 0 and no bias the processed row is
 * the raw row bit for bit.  The bias list of row b is bias_ids / bias_values
 * [b][HPA_LOGIT_BIAS_MAX], its first bias_n[b] entries (ids distinct and in
 * [0, V); an id outside is ignored; bias_n NULL: no list).
 * Outputs: processed [B][V] (nullable) and, per (slice, row), the slice's
 * (max, argmax) at part[(slice * Mp + b) * 2] (value, then the column's bits) --
 * the layout hpa_argmax_final reads with ntiles = slices; the larger value
 * wins, then the lower column; a slice without a value above -inf leaves
 * (-inf, INT_MAX), so a row with none gets id 0 (part nullable).  active as
 * hpa_argmax_final: an inactive row keeps its processed row and its partials.
 * slices: column ranges per row, one workgroup each (<= 0: by
 * hpa_logits_process_slices on this device); a slice may hold at most 65528
 * columns.  Reductions run in a fixed order: a launch repeats bit for bit. */
#define HPA_LOGIT_BIAS_MAX 300
int hpa_logits_process(const float* logits, int B, int V, const unsigned short* counts, const float* repetition,
                       const float* presence, const float* frequency, const int* bias_ids, const float* bias_values,
                       const int* bias_n, const int* active, float* processed, float* part, int Mp, int slices);
/* slices per row for hpa_logits_process, pure host arithmetic: about four
 * workgroups per CU over the launch (B = 8 still fills 256 CUs, B = 64 is not
 * split further than that), no slice under 1024 columns, none over the limit
 * above.  0 on bad arguments; num_cus <= 0 counts as 256. */
int hpa_logits_process_slices(int B, int V, int num_cus);
/* R fed tokens: history[seq[i]][pos[i]] = tok[i] (history [B][max_ctx]) and,
 * where pos[i] >= from_pos[seq[i]], counts[seq[i]][tok[i]] += 1 (an integer
 * atomic: the sums do not depend on the order).  seq NULL: row i is sequence
 * i.  A row outside the tables is skipped.  max_ctx <= 65535. */
int hpa_token_record(int* history, int max_ctx, unsigned short* counts, int V, int B, const int* from_pos,
                     const int* seq, const int* pos, const int* tok, int R);
/* counts[seq][*] = 0, then += 1 for every history[seq][p], from <= p < n
 * (n <= from: the row is only zeroed) */
int hpa_token_recount(const int* history, int max_ctx, unsigned short* counts, int V, int seq, int from, int n);
/* paged decode attention writing its output in frag layout ([B][C]) */
int hpa_paged_attention_decode_frag(const float* q, const HpaKVPool* pool, int layer,
                                    const int* block_table, int bt_stride, const int* pos,
                                    float* out_frag, int B);

/* ---------------- prefill (multi-query) ----------------
 * attention_paged (paged_infer.c:163-240) for T query rows per sequence at
 * absolute positions start[b] + t, causal over the sequence's pages: q
 * [B*T][C] row-major (row = b*T + t), out frag layout [ceil16(B*T)][C].
 * S = QK^T and O += PV on v_mfma_f32_16x16x4_f32 (dense here), online
 * softmax from the reference's -10000 floor.  The K/V of every query
 * position must already be in the pages (the prefill QKV GEMM appends them). */
int hpa_paged_attention_prefill(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                int bt_stride, const int* start, int B, int T, float* out_frag);
/* ragged form (continuous batching): sequence b has len[b] >= 0 query rows
 * starting at row row0[b] of q / out (device arrays, given together);
 * T = max(len).  row0 = len = NULL is the uniform form above. */
int hpa_paged_attention_prefill_ragged(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                       int bt_stride, const int* start, const int* row0, const int* len, int B,
                                       int T, float* out_frag);
/* ---------------- speculative decoding (hpa_verify.hip) ----------------
 * The attention of a verify pass: the ragged contract above (q [rows][C]
 * row-major, row row0[b] + t at position start[b] + t sees keys 0 ..
 * start[b] + t, frag output, len[b] == 0 skipped, softmax from the -10000
 * floor) for 1 <= T = max(len) <= HPA_VERIFY_MAX_ROWS query rows per sequence
 * over a long context.  The decode kernel's structure: one workgroup per
 * (sequence, head), 64-token K/V tiles streamed once into registers and used
 * for every row, queries broadcast from LDS, wave states folded in wave order
 * (a launch repeats bit for bit); 4 or 8 waves per workgroup as
 * hpa_attn_pick_waves says, or as hpa_set_attention_waves(4 or 8) names them.
 * fp32 pools, head size 64, page size 8, 16,
 * 32 or 64, no context splits; anything else returns nonzero and launches
 * nothing (bf16 / fp8 pools: hpa_paged_attention_prefill_ragged). */
#define HPA_VERIFY_MAX_ROWS 8
int hpa_paged_attention_verify(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                               int bt_stride, const int* start, const int* row0, const int* len, int B,
                               int T, float* out_frag);
/* row tables of a verify pass (device arrays): row row0[b] of sequence b with
 * len[b] > 0 is its pending id next[b], rows row0[b] + 1 .. + len[b] - 1 its
 * drafts drafts[draft0[b] ..]; tok / pos / seq: the row's token, position
 * start[b] + t and sequence; target: the next row's token (the id the row must
 * predict for that draft to be accepted), -1 for a sequence's last row */
int hpa_verify_rows(const int* next, const int* drafts, const int* draft0, const int* start, const int* row0,
                    const int* len, int B, int* tok, int* pos, int* seq, int* target);
/* the accept decision from the rows' greedy ids top_id: n_accepted[b] = the
 * largest a with tok[row0[b] + i] == top_id[row0[b] + i - 1] for 1 <= i <= a;
 * cont_row[b] = row0[b] + a, the row decoding continues from; pos[b] =
 * start[b] + a (the pick that follows advances it by one).  len[b] == 0:
 * n_accepted[b] = cont_row[b] = -1, pos[b] untouched. */
int hpa_verify_accept(const int* tok, const int* top_id, const int* start, const int* row0, const int* len, int B,
                      int* n_accepted, int* cont_row, int* pos);

/* ---------------- tree speculation (hpa_verify.hip) ----------------
 * The len[b] <= HPA_VERIFY_MAX_ROWS rows of sequence b are the nodes of a token
 * tree, not a chain: node 0 is the pending id, node j + 1 is draft j (packed
 * like `drafts`) and hangs from node parents[draft0[b] + j] in [0, j] -- a
 * smaller index than its own, so node order is topological.  Node i's K/V is
 * appended to slot start[b] + i whatever its depth.
 *
 * hpa_paged_attention_verify_tree: hpa_paged_attention_verify's contract with
 * one change: the row of node r of sequence b sees keys 0 .. start[b] - 1 plus
 * key start[b] + i for every bit i of anc[row0[b] + r] (device, one byte per
 * packed row; bit r itself must be set and no bit above it, as
 * hpa_verify_tree_rows writes them).  The same kernel with a compile-time mask
 * test: same tile loop, same dealing of tiles over waves, same fold, so with
 * chain masks (bits 0 .. r) the output bits are hpa_paged_attention_verify's.
 * Each wave reads its sequence's masks once into scalar registers.  A hidden
 * node's K/V is still streamed and its V row multiplied by a weight of
 * exactly 0: hidden slots must hold finite values (the pass's own appends do).
 * Limits as the verify kernel's: fp32 pool, head size 64, page size 8 / 16 /
 * 32 / 64, 1 <= T <= HPA_VERIFY_MAX_ROWS, no context splits; anything else
 * returns nonzero and launches nothing. */
int hpa_paged_attention_verify_tree(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                    int bt_stride, const int* start, const int* row0, const int* len,
                                    const unsigned char* anc, int B, int T, float* out_frag);
/* row tables of a tree pass (device arrays), the sibling of hpa_verify_rows:
 * per packed row row0[b] + i of node i: tok (next[b] for node 0, else draft
 * i - 1), seq = b, pos = start[b] + depth(i) (what hpa_embed_frag reads for
 * wpe), slot = start[b] + i (the QKV GEMM's append position) and anc (bit k:
 * node k is node i or one of its ancestors).  A parent outside [0, j] is
 * clamped into it (the engine refuses it before launching anything). */
int hpa_verify_tree_rows(const int* next, const int* drafts, const int* parents, const int* draft0, const int* start,
                         const int* row0, const int* len, int B, int* tok, int* pos, int* seq, int* slot,
                         unsigned char* anc);
/* the accept walk, one thread per sequence: cur = 0; while some child c of cur
 * (lowest index first) has tok[row0[b] + c] == top_id[row0[b] + cur]: cur = c.
 * n_accepted[b] = a = depth(cur); path[b * HPA_VERIFY_MAX_ROWS + i], i < a:
 * the node indices walked (strictly increasing); cont_row[b] = row0[b] + cur;
 * pos[b] = start[b] + a.  len[b] == 0: n_accepted[b] = cont_row[b] = -1, pos[b]
 * and path untouched.  Siblings with equal tokens: the lower index wins (the
 * engine refuses such trees). */
int hpa_verify_tree_accept(const int* tok, const int* top_id, const int* parents, const int* draft0, const int* start,
                           const int* row0, const int* len, int B, int* n_accepted, int* path, int* cont_row,
                           int* pos);
/* K/V compaction after a tree pass: for every sequence b with a =
 * n_accepted[b] > 0 and every k = 1 .. a with p = path[b * HPA_VERIFY_MAX_ROWS +
 * k - 1] != k, the K and V of slot start[b] + p go to slot start[b] + k, in
 * every layer and head; pages are resolved through the block table (source and
 * destination may lie in different pages).  ONE asynchronous launch on the
 * current stream; start / path / n_accepted / block_table are device arrays.
 * In place: each thread owns a fixed (layer, K|V, head, 4 dims) lane and walks
 * k upwards; path strictly increases with path[k-1] >= k, so a destination is
 * never a source still to be read.  Entries that break that, and n_accepted
 * <= 0, move nothing.  The slots from start[b] on must be private to b (the
 * engine's appends went there after its copy-on-write).  fp32 pools, head size
 * 64; anything else returns nonzero and launches nothing. */
int hpa_pool_compact_path(const HpaKVPool* pool, const int* block_table, int bt_stride, const int* start,
                          const int* path, const int* n_accepted, int B);

/* rows[i] of a frag-layout [src_Mp][C] matrix and of its LN statistics
 * ([C/16][src_Mp][2]) -> row i of dst / dst_stats (n rows; prefill -> logits);
 * rows[i] < 0 leaves row i of dst as it is */
int hpa_gather_rows_frag(const float* src, const float* src_stats, int src_Mp, const int* rows, int n,
                         float* dst, float* dst_stats, int dst_Mp, int C);

/* ---------------- multi-GPU: RCCL over xGMI (hpa_comm.hip) ----------------
 * One process per GPU.  Rank 0 makes the id
 * (hpa_comm_unique_id), the launcher hands it to every rank (any out-of-band
 * channel: a file -- bench.py --, sockets, MPI), and each rank binds its
 * current device with hpa_comm_init.  The decode engine's end-of-step gather
 * (gpt2_decode_gather) runs on it. */
size_t hpa_comm_id_bytes(void);                     /* sizeof(ncclUniqueId) = 128 */
int    hpa_comm_unique_id(void* id, size_t id_bytes);
int    hpa_comm_init(int nranks, int rank, const void* id);
int    hpa_comm_destroy(void);
int    hpa_comm_size(void);                         /* 0 before hpa_comm_init */
int    hpa_comm_rank(void);                         /* -1 before hpa_comm_init */
/* root receives every rank's bytes in rank order (ncclSend/ncclRecv group;
 * uneven sizes allowed) on `stream` (NULL = the library stream), async */
int    hpa_comm_gatherv(const void* send, size_t send_bytes, void* recv, const size_t* bytes_per_rank, int root,
                        void* stream);
/* the gather's layout, host arithmetic only (what hpa_comm_gatherv posts):
 * recv_off[r] = byte offset of rank r's rows in root's buffer (rank order);
 * returns the number of ncclRecv the root posts (ranks != root with bytes),
 * or 1 / 0 on a non-root rank (it sends iff its bytes are nonzero); -1 on bad
 * arguments.  *own_off = root's own rows' offset (its local copy). */
int    hpa_comm_gather_layout(int nranks, int rank, int root, const size_t* bytes_per_rank, size_t* recv_off,
                              size_t* own_off);
/* the gather's schedule, host arithmetic only: the point-to-point operations
 * THIS rank posts for one hpa_comm_gatherv, in posting order.  hpa_comm_gatherv
 * executes exactly this list (ncclSend / ncclRecv inside one NCCL group, then
 * the root's local copy), so a host transport can run the same schedule (the
 * world-size-2..4 gloo tests, tests/test_multi_rank.py).  SEND: send_bytes of
 * the send buffer to `peer` (offset 0); RECV: `bytes` from `peer` at `offset`
 * of recv; COPY (root): its own rows into recv at `offset`.  Zero-byte
 * operations are never listed.  Returns the operation count (<= nranks), -1 on
 * bad arguments or when max_ops is too small (ops may be NULL to count). */
enum { HPA_COMM_SEND = 0, HPA_COMM_RECV = 1, HPA_COMM_COPY = 2 };
typedef struct {
    int op;        /* HPA_COMM_* */
    int peer;      /* the other rank (COPY: this rank) */
    size_t offset; /* byte offset in recv (SEND: 0, in send) */
    size_t bytes;
} HpaCommOp;
int    hpa_comm_gather_plan(int nranks, int rank, int root, const size_t* bytes_per_rank, HpaCommOp* ops,
                            int max_ops);
/* timing helpers over the communicator (RCCL all-reduce on the library
 * stream, then a host wait): a barrier, and the maximum of one host double
 * over the ranks (bench.py's max-over-ranks step time) */
int    hpa_comm_barrier(void);
int    hpa_comm_allreduce_max(double* value);
/* single-process form (one process driving ndev GPUs,
 * ncclCommInitAll): communicators for devices devs[0..ndev-1], rank i =
 * devs[i]; hpa_comm_use(i) makes comm i (and device devs[i]) current for the
 * calls above.  Exclusive with hpa_comm_init. */
int    hpa_comm_init_all(int ndev, const int* devs);
int    hpa_comm_use(int index);
/* ncclGroupStart / ncclGroupEnd around the collectives posted between them
 * (the single-process form: every device's gather from one thread) */
int    hpa_comm_group_start(void);
int    hpa_comm_group_end(void);

/* ---------------- reference-layout kernels (drop-in compat) ----------------
 * Pages in the reference layout: token-major [block_size][C] per page
 * (block_manager.c:145-146).  key_blocks/value_blocks: DEVICE arrays of
 * DEVICE page pointers.  Reference arithmetic order (no FMA contraction), so
 * results match the reference bit-for-bit up to expf/tanhf ulps. */
int hpa_ref_attention_paged(float* out, float* preatt, float* att, const float* inp,
                            float* const* key_blocks, float* const* value_blocks, int B, int T,
                            int C, int NH, int offset, int block_size);
/* cached == 0: matmul_forward (:92-114); cached == 1: matmul_cached
 * (:117-160): rows t < T-1 compute only the first C outputs (Q) */
int hpa_ref_matmul(float* out, const float* inp, const float* weight, const float* bias, int B,
                   int T, int C, int OC, int cached);
int hpa_ref_layernorm(float* out, float* mean, float* rstd, const float* inp, const float* weight,
                      const float* bias, int N, int C);
int hpa_ref_encoder(float* out, const int* inp, const float* wte, const float* wpe, int B, int T,
                    int C, int pos_offset);
int hpa_ref_gelu(float* out, const float* inp, int N);
int hpa_ref_residual(float* out, const float* a, const float* b, int N);
int hpa_ref_softmax(float* probs, const float* logits, int N, int V);

#ifdef __cplusplus
}
#endif
#endif
