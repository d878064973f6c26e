"""Python host mirror of libpaged_hip.so (ctypes over the C-ABI).

This is a thin binding, not a compute path: every call lands in the C
library (include/hip_paged_attn.h, paged_infer.h, block_manager.h), which
runs the MI355X kernels.  There is no fallback: if the library is missing or
no HIP device is visible, the calls raise.

Names mirror the reference API (paged_infer.c / block_manager.c of
mx60s/llm.c-paged): Model wraps GPT2 + gpt2_decode_* (the decode hot path),
BlockManager wraps create_block_manager / request_block / ... .
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HPA_LIB") or os.path.join(HERE, "libpaged_hip.so")  # HPA_LIB: tool A/B builds
INCLUDE_DIR = os.path.join(os.path.dirname(HERE), "include")

_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
_V = ctypes.c_void_p


class GPT2Config(ctypes.Structure):
    """paged_infer.c:397-403"""
    _fields_ = [("max_seq_len", ctypes.c_int), ("vocab_size", ctypes.c_int),
                ("num_layers", ctypes.c_int), ("num_heads", ctypes.c_int),
                ("channels", ctypes.c_int)]

    def as_dict(self):
        return dict(maxT=self.max_seq_len, V=self.vocab_size, L=self.num_layers,
                    NH=self.num_heads, C=self.channels)


class KVBlock(ctypes.Structure):
    """block_manager.c:9-15"""
    _fields_ = [("keys", _F), ("values", _F), ("filled", ctypes.c_int),
                ("prompt_id", ctypes.c_int), ("lru_counter", ctypes.c_int)]


class HpaKVPool(ctypes.Structure):
    _fields_ = [("base", _V), ("num_layers", ctypes.c_int), ("num_heads", ctypes.c_int),
                ("head_size", ctypes.c_int), ("page_size", ctypes.c_int),
                ("num_pages", ctypes.c_int), ("dtype", ctypes.c_int),
                ("elem_bytes", ctypes.c_size_t), ("page_elems", ctypes.c_size_t),
                ("layer_elems", ctypes.c_size_t), ("bytes", ctypes.c_size_t),
                ("managed", ctypes.c_int), ("scales", _F)]


class HpaFusedGemm(ctypes.Structure):
    _fields_ = [("x", _V), ("M", ctypes.c_int), ("K", ctypes.c_int), ("ln_stats", _V),
                ("ln_ntiles", ctypes.c_int), ("ln_w", _V), ("ln_b", _V), ("w", _V),
                ("N", ctypes.c_int), ("bias", _V), ("epilogue", ctypes.c_int), ("out", _V),
                ("res_in", _V), ("stats_out", _V), ("part_out", _V),
                ("pool", ctypes.POINTER(HpaKVPool)), ("layer", ctypes.c_int), ("block_table", _V),
                ("bt_stride", ctypes.c_int), ("pos", _V), ("waves", ctypes.c_int),
                ("row_blocks", ctypes.c_int), ("variant", ctypes.c_int), ("col_tiles", ctypes.c_int),
                ("row_seq", _V), ("ln_fold_c1", _V), ("sk_slab", _V), ("sk_count", _V),
                ("w_dtype", ctypes.c_int), ("pick_next", _V), ("pick_tokens", _V), ("pick_pos", _V),
                ("pick_count", _V), ("score_target", _V), ("score_part", _V)]


class HpaChainB16Args(ctypes.Structure):
    """include/hip_paged_attn.h HpaChainB16Args, member for member (the bf16-weight
    decode chain, hpa_chain_b16.hip)"""
    _fields_ = [("B", ctypes.c_int), ("layer", ctypes.c_int), ("last", ctypes.c_int),
                ("pool", ctypes.POINTER(HpaKVPool)), ("block_table", _V), ("bt_stride", ctypes.c_int),
                ("pos", _V), ("att", _V), ("res", _V), ("res2", _V), ("fch", _V),
                ("w_ap", _V), ("w_fc", _V), ("w_fp", _V), ("w_qkv", _V),
                ("b_ap", _V), ("ln2_w", _V), ("ln2_b", _V), ("b_fc", _V), ("b_fp", _V),
                ("ln1_w", _V), ("ln1_b", _V), ("b_qkv", _V),
                ("q_out", _V), ("stats_out", _V), ("stats_mp", ctypes.c_int), ("slab", _V),
                ("counters", _V), ("err", _V), ("err_sticky", _V)]


HPA_FEPI_QKV, HPA_FEPI_RESID, HPA_FEPI_GELU, HPA_FEPI_LOGITS, HPA_FEPI_SCORE = 0, 1, 2, 3, 4
HPA_COMM_SEND, HPA_COMM_RECV, HPA_COMM_COPY = 0, 1, 2


class HpaCommOp(ctypes.Structure):
    """include/hip_paged_attn.h HpaCommOp: one operation of the gather schedule"""
    _fields_ = [("op", ctypes.c_int), ("peer", ctypes.c_int), ("offset", ctypes.c_size_t),
                ("bytes", ctypes.c_size_t)]


def frag_index(m, k, K):
    """numpy mirror of hpa_internal.h frag_index (vectorised over m, k)"""
    m = np.asarray(m)
    k = np.asarray(k)
    return ((((m >> 4) * (K >> 4) + (k >> 4)) * 64 + ((m & 15) + 16 * ((k >> 2) & 3))) << 2) + (k & 3)


def to_frag(a, pad=16):
    """host [rows][K] -> frag-layout flat array (rows padded to `pad`)"""
    rows, K = a.shape
    rp = (rows + pad - 1) // pad * pad
    out = np.zeros(rp * K, np.float32)
    m, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
    out[frag_index(m, k, K)] = a
    return out


def from_frag(f, rows, K):
    m, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
    return f[frag_index(m, k, K)]


def frag_bf16_index(m, k, K):
    """element (m, k) of a [rows][K] matrix in the bf16 frag layout (hip_paged_attn.h;
    vectorised over m, k): the 16-byte fragment of lane m % 16 + 16 * ((k % 16) / 4) of
    (row block m / 16, 32-deep step k / 32), half (k % 32) / 16 of it"""
    m = np.asarray(m)
    k = np.asarray(k)
    return ((((m >> 4) * (K >> 5) + (k >> 5)) * 64 + ((m & 15) + 16 * ((k >> 2) & 3))) << 3) + (k & 3) + \
        4 * ((k >> 4) & 1)


def from_frag_bf16(bits_u16, rows, K):
    """bf16 frag layout (hpa_pack_frag_bf16, the chain's fch) -> [rows][K] bf16 bit patterns"""
    m, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
    return np.asarray(bits_u16, np.uint16)[frag_bf16_index(m, k, K)]


GPT2_124M = dict(maxT=1024, V=50257, L=12, NH=12, C=768)
GPT2_XL = dict(maxT=1024, V=50257, L=48, NH=25, C=1600)

def config(d):
    return GPT2Config(d["maxT"], d["V"], d["L"], d["NH"], d["C"])


def gather_plan(nranks, rank, root, nbytes):
    """hpa_comm_gather_plan: the (op, peer, offset, bytes) operations this rank
    posts for one end-of-step gather -- the list hpa_comm_gatherv executes over
    RCCL (host arithmetic, no GPU needed)"""
    L = lib()
    b = (ctypes.c_size_t * nranks)(*nbytes)
    ops = (HpaCommOp * nranks)()
    n = L.hpa_comm_gather_plan(nranks, rank, root, b, ops, nranks)
    if n < 0:
        raise ValueError("hpa_comm_gather_plan: bad arguments")
    return [(o.op, o.peer, o.offset, o.bytes) for o in ops[:n]]


def build(force=False):
    """Compile libpaged_hip.so in-tree (hipcc --offload-arch=gfx950)."""
    cmd = ["make", "-s", "-C", HERE, "-j8"]
    if force:
        cmd.insert(2, "-B")
    subprocess.run(cmd, check=True)
    return LIB_PATH


_lib = None


def _sig(L, name, res, args):
    f = getattr(L, name)
    f.restype = res
    f.argtypes = args


def lib():
    """Load libpaged_hip.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} missing: run __graft_entry__.build() (no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    i, v, f, sz = ctypes.c_int, _V, ctypes.c_float, ctypes.c_size_t
    P = ctypes.POINTER(HpaKVPool)
    # runtime
    _sig(L, "hpa_init", i, [i])
    _sig(L, "hpa_device_count", i, [])
    _sig(L, "hpa_get_device", i, [])
    _sig(L, "hpa_set_stream", i, [v])
    _sig(L, "hpa_get_stream", v, [])
    _sig(L, "hpa_synchronize", i, [])
    _sig(L, "hpa_device_synchronize", i, [])
    _sig(L, "hpa_malloc", v, [sz])
    _sig(L, "hpa_malloc_managed", v, [sz])
    _sig(L, "hpa_host_alloc", v, [sz])
    _sig(L, "hpa_free", i, [v])
    _sig(L, "hpa_host_free", i, [v])
    _sig(L, "hpa_memcpy", i, [v, v, sz])
    _sig(L, "hpa_memcpy_async", i, [v, v, sz])
    _sig(L, "hpa_memset_async", i, [v, i, sz])
    _sig(L, "hpa_is_device_accessible", i, [v])
    _sig(L, "hpa_event_create", v, [])
    _sig(L, "hpa_event_record", i, [v])
    _sig(L, "hpa_event_elapsed_ms", f, [v, v])
    _sig(L, "hpa_event_destroy", i, [v])
    _sig(L, "hpa_event_create_nt", v, [])
    _sig(L, "hpa_stream_create", v, [])
    _sig(L, "hpa_stream_destroy", i, [v])
    _sig(L, "hpa_stream_wait_event", i, [v])
    _sig(L, "hpa_event_synchronize", i, [v])
    _sig(L, "hpa_last_error", ctypes.c_char_p, [])
    _sig(L, "hpa_build_flags", i, [])
    _sig(L, "hpa_device_info", i, [ctypes.c_char_p, i, _I, ctypes.POINTER(sz)])
    _sig(L, "hpa_set_attention_waves", i, [i])
    _sig(L, "hpa_attn_pick_waves", i, [i, i, i, i])
    # pool + kernels
    _sig(L, "hpa_pool_create", i, [P, i, i, i, i, i, i, i])
    _sig(L, "hpa_pool_destroy", None, [P])
    _sig(L, "hpa_pool_set_scales", i, [P, _F, _F])
    _sig(L, "hpa_pool_tile", v, [P, i, i, i, i])
    _sig(L, "hpa_pool_k_index", sz, [P, i, i, i, i, i])
    _sig(L, "hpa_pool_v_index", sz, [P, i, i, i, i, i])
    _sig(L, "hpa_pool_fill_random", i, [P, v, i, i, i, ctypes.c_uint64])
    _sig(L, "hpa_paged_attention_decode", i, [v, P, i, v, i, v, v, i])
    _sig(L, "hpa_attn_ws_bytes", sz, [i, i, i])
    _sig(L, "hpa_attn_pick_splits", i, [i, i, i, i])
    _sig(L, "hpa_paged_attention_decode_split", i, [v, P, i, v, i, v, v, i, i, v, i])
    _sig(L, "hpa_paged_attention_decode_split_w", i, [v, P, i, v, i, v, v, i, i, v, i, i])
    _sig(L, "hpa_attn_shared_ws_bytes", sz, [i, i, i])
    _sig(L, "hpa_attn_shared_pick_splits", i, [i, i, i, i])
    _sig(L, "hpa_paged_attention_decode_shared", i, [v, P, i, v, i, v, v, i, v, v, i, v, i, v, i, i])
    _sig(L, "hpa_comm_id_bytes", sz, [])
    _sig(L, "hpa_comm_unique_id", i, [v, sz])
    _sig(L, "hpa_comm_init", i, [i, i, v])
    _sig(L, "hpa_comm_destroy", i, [])
    _sig(L, "hpa_comm_size", i, [])
    _sig(L, "hpa_comm_rank", i, [])
    _sig(L, "hpa_comm_gatherv", i, [v, sz, v, ctypes.POINTER(sz), i, v])
    _sig(L, "hpa_comm_gather_layout", i, [i, i, i, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(sz)])
    _sig(L, "hpa_comm_gather_plan", i, [i, i, i, ctypes.POINTER(sz), ctypes.POINTER(HpaCommOp), i])
    _sig(L, "hpa_comm_barrier", i, [])
    _sig(L, "hpa_comm_allreduce_max", i, [ctypes.POINTER(ctypes.c_double)])
    _sig(L, "hpa_comm_init_all", i, [i, ctypes.POINTER(i)])
    _sig(L, "hpa_comm_use", i, [i])
    _sig(L, "hpa_ref_attention_paged", i, [v, v, v, v, v, v, i, i, i, i, i, i])
    _sig(L, "hpa_ref_matmul", i, [v, v, v, v, i, i, i, i, i])
    # block manager (block_manager.c API)
    _sig(L, "create_block_manager", v, [i])
    _sig(L, "create_block_manager_ex", v, [i, i, i, i, i])
    _sig(L, "destroy_block_manager", None, [v])
    _sig(L, "request_block", ctypes.POINTER(KVBlock), [v, i])
    _sig(L, "get_current_block", ctypes.POINTER(KVBlock), [v, i])
    _sig(L, "free_blocks_for_prompt", None, [v, i])
    _sig(L, "find_least_recently_used_block", i, [v])
    _sig(L, "page_out_lru_block", None, [v])
    _sig(L, "get_next_block_id", i, [v, i, i])
    _sig(L, "collect_kv_blocks", v, [v, i, _I])
    _sig(L, "bm_block_index", i, [v, v])
    _sig(L, "bm_free_pages", i, [v])
    _sig(L, "bm_use_host_pages", None, [v])
    _sig(L, "bm_default_backend_kind", i, [])
    _sig(L, "bm_fork_prompt", i, [v, i, i, i])
    _sig(L, "bm_make_private", i, [v, i, i, _I])
    _sig(L, "bm_page_refs", i, [v, i])
    _sig(L, "bm_shared_pages", i, [v])
    _sig(L, "hpa_pool_copy_pages", i, [P, _I, _I, i])
    _sig(L, "hpa_park_bytes", sz, [P, i])
    _sig(L, "hpa_park_offset", sz, [P, i, i, i])
    _sig(L, "hpa_pool_gather_pages", i, [P, _I, i, v])
    _sig(L, "hpa_pool_scatter_pages", i, [P, _I, i, v])
    _sig(L, "hpa_park_set_nontemporal", i, [i])
    _sig(L, "hpa_park_nontemporal", i, [])
    _sig(L, "gpt2_decode_park", v, [v, i, i])
    _sig(L, "gpt2_decode_unpark", i, [v, v, i])
    _sig(L, "gpt2_parked_tokens", i, [v])
    _sig(L, "gpt2_parked_bytes", sz, [v])
    _sig(L, "gpt2_parked_free", None, [v])
    _sig(L, "gpt2_decode_fork", i, [v, i, i, i])
    _sig(L, "gpt2_decode_free_pages", i, [v])
    _sig(L, "gpt2_decode_page_slots", i, [v, _I, i])
    # model + decode engine
    _sig(L, "gpt2_alloc", v, [])
    _sig(L, "gpt2_release", None, [v])
    _sig(L, "gpt2_set_manager", None, [v, v])
    _sig(L, "gpt2_acts_logits", _F, [v])
    _sig(L, "gpt2_acts_probs", _F, [v])
    _sig(L, "gpt2_num_parameters", sz, [GPT2Config])
    _sig(L, "gpt2_synthetic_params", i, [GPT2Config, ctypes.c_ulonglong, _F])
    _sig(L, "gpt2_write_checkpoint", i, [ctypes.c_char_p, GPT2Config, _F])
    _sig(L, "gpt2_write_checkpoint_ex", i, [ctypes.c_char_p, GPT2Config, _F, i])
    _sig(L, "gpt2_read_checkpoint", i, [ctypes.c_char_p, ctypes.POINTER(GPT2Config), _F])
    _sig(L, "tokenizer_init", None, [v, ctypes.c_char_p])
    _sig(L, "tokenizer_decode", ctypes.c_char_p, [v, ctypes.c_uint32])
    _sig(L, "tokenizer_free", None, [v])
    _sig(L, "safe_printf", None, [ctypes.c_char_p])
    _sig(L, "gpt2_build_from_params", i, [v, GPT2Config, _F])
    _sig(L, "gpt2_build_synthetic", i, [v, GPT2Config, ctypes.c_ulonglong])
    _sig(L, "gpt2_build_from_checkpoint", None, [v, ctypes.c_char_p])
    _sig(L, "gpt2_forward", None, [v, _I, _I, sz, sz, sz, i])
    _sig(L, "gpt2_decode_init", i, [v, i, i, i])
    _sig(L, "gpt2_decode_init_ex", i, [v, i, i, i, i])
    _sig(L, "gpt2_decode_init_w", i, [v, i, i, i, i, i])
    _sig(L, "hpa_pack_frag_bf16", i, [v, i, i, i, v])
    _sig(L, "hpa_frag_bf16_elems", ctypes.c_size_t, [i, i])
    _sig(L, "gpt2_decode_prefill", i, [v, _I, i, _I])
    _sig(L, "gpt2_decode_prefill_ragged", i, [v, _I, _I, _I])
    _sig(L, "gpt2_decode_score", i, [v, _I, _I, _I, _F, _I, _I])
    _sig(L, "gpt2_decode_set_score_chunk", i, [v, i])
    _sig(L, "gpt2_decode_set_logprobs", i, [v, i])
    _sig(L, "gpt2_decode_logprobs", i, [v, _F])
    _sig(L, "hpa_score_workspace", i, [i, i, ctypes.POINTER(ctypes.c_size_t)])
    _sig(L, "hpa_score_final", i, [v, i, i, i, v, v, v, v])
    _sig(L, "hpa_logprob_rows", i, [v, i, i, v, v, v])
    _sig(L, "gpt2_decode_set_top_logprobs", i, [v, i])
    _sig(L, "gpt2_decode_top_logprobs_k", i, [v])
    _sig(L, "gpt2_decode_top_logprobs", i, [v, _I, _F])
    _sig(L, "gpt2_decode_score_top", i, [v, _I, _I, _I, _F, i, _I, _F, _I])
    _sig(L, "hpa_top_logprobs", i, [v, i, i, i, v, v, v, v, v, v])
    _sig(L, "hpa_top_logprobs_workspace", i, [i, i, i, ctypes.POINTER(ctypes.c_size_t)])
    _sig(L, "hpa_top_logprobs_ws", i, [v, i, i, i, v, v, v, v, v, v, v, ctypes.c_size_t, i])
    _sig(L, "hpa_top_logprobs_slices", i, [i, i, i])
    _sig(L, "gpt2_decode_release", i, [v, i])
    _sig(L, "gpt2_decode_set_sampling", i, [v, i, ctypes.c_ulonglong])
    _sig(L, "gpt2_decode_set_sampling_params", i, [v, i, ctypes.c_float, i, ctypes.c_float])
    _sig(L, "gpt2_decode_sampling_params", i, [v, i, _F, _I, _F])
    _sig(L, "gpt2_decode_seed_sequence", i, [v, i, ctypes.c_ulonglong])
    _sig(L, "gpt2_decode_sampler_state", i, [v, i, ctypes.POINTER(ctypes.c_ulonglong)])
    _sig(L, "gpt2_decode_set_processors", i, [v, i])
    _sig(L, "gpt2_decode_processors", i, [v])
    _sig(L, "gpt2_decode_set_penalties", i, [v, i, ctypes.c_float, ctypes.c_float, ctypes.c_float, i])
    _sig(L, "gpt2_decode_penalties", i, [v, i, _F, _F, _F, _I])
    _sig(L, "gpt2_decode_set_logit_bias", i, [v, i, _I, _F, i])
    _sig(L, "gpt2_decode_logit_bias", i, [v, i, _I, _F, _I])
    _sig(L, "gpt2_decode_processed_logits", v, [v])
    _sig(L, "gpt2_decode_history", i, [v, i, _I, _I])
    _sig(L, "gpt2_decode_token_counts", i, [v, i, _I])
    _sig(L, "hpa_logits_process", i, [v, i, i, v, v, v, v, v, v, v, v, v, v, i, i])
    _sig(L, "hpa_logits_process_slices", i, [i, i, i])
    _sig(L, "hpa_token_record", i, [v, i, v, i, i, v, v, v, v, i])
    _sig(L, "hpa_token_recount", i, [v, i, v, i, i, i, i])
    _sig(L, "hpa_paged_attention_prefill", i, [_F, v, i, _I, i, _I, i, i, _F])
    _sig(L, "hpa_paged_attention_prefill_ragged", i, [_F, v, i, _I, i, _I, _I, _I, i, i, _F])
    _sig(L, "hpa_gather_rows_frag", i, [_F, _F, i, _I, i, _F, _F, i, i])
    _sig(L, "hpa_attention_waves", i, [])
    _sig(L, "hpa_paged_attention_verify", i, [_F, v, i, _I, i, _I, _I, _I, i, i, _F])
    _sig(L, "hpa_verify_rows", i, [_I, _I, _I, _I, _I, _I, i, _I, _I, _I, _I])
    _sig(L, "hpa_verify_accept", i, [_I, _I, _I, _I, _I, i, _I, _I, _I])
    _sig(L, "gpt2_decode_verify", i, [v, _I, _I, _I, _I, _F])
    _sig(L, "gpt2_decode_verify_sampled", i, [v, _I, _I, _I, _I, _F])
    _sig(L, "gpt2_decode_verify_plan", i, [i, i, i, i, i])
    _sig(L, "gpt2_decode_set_verify_attention", i, [v, i])
    _sig(L, "gpt2_attn_shared_plan", i, [_I, i, _I, i, i, i, i, i, _I, _I, _I])
    _sig(L, "gpt2_decode_set_shared_attention", i, [v, i])
    _sig(L, "gpt2_decode_shared_attention", i, [v])
    _sig(L, "gpt2_decode_shared_plan", i, [v, _I, _I])
    _sig(L, "gpt2_decode_set_shared_thresholds", i, [v, i, i, i])
    _sig(L, "gpt2_decode_shared_thresholds", i, [v, _I, _I, _I])
    _sig(L, "gpt2_decode_shared_splits", i, [v])
    _sig(L, "gpt2_decode_set_shared_splits", i, [v, i])
    _sig(L, "gpt2_ngram_draft", i, [_I, i, i, i, i, _I])
    _U8 = ctypes.POINTER(ctypes.c_ubyte)
    _sig(L, "hpa_paged_attention_verify_tree", i, [_F, v, i, _I, i, _I, _I, _I, _U8, i, i, _F])
    _sig(L, "hpa_verify_tree_rows", i, [_I, _I, _I, _I, _I, _I, _I, i, _I, _I, _I, _I, _U8])
    _sig(L, "hpa_verify_tree_accept", i, [_I, _I, _I, _I, _I, _I, _I, i, _I, _I, _I, _I])
    _sig(L, "hpa_pool_compact_path", i, [P, _I, i, _I, _I, _I, i])
    _sig(L, "gpt2_decode_verify_tree", i, [v, _I, _I, _I, _I, _I, _I])
    _sig(L, "gpt2_ngram_draft_tree", i, [_I, i, i, i, i, i, i, _I, _I])
    _sig(L, "gpt2_decode_verify_tree_sampled", i, [v, _I, _I, _I, _I, _I, _I, _F])
    _sig(L, "gpt2_tree_dense_tables", i, [_I, _I, _I, i, _I, _I, _I, _I, _I, _I])
    _sig(L, "gpt2_decode_step", i, [v, _I, _I])
    _sig(L, "gpt2_decode_step_async", i, [v, _I])
    _sig(L, "gpt2_decode_step_traced", i, [v, _I, _I, _F])
    _sig(L, "gpt2_decode_trace_next_pass", i, [v, _F, ctypes.c_size_t])
    _sig(L, "gpt2_decode_reset", i, [v])
    _sig(L, "gpt2_decode_fill_random", i, [v, i, ctypes.c_ulonglong])
    _sig(L, "gpt2_decode_set_graph", i, [v, i])
    _sig(L, "gpt2_decode_reserve", i, [v, i])
    _sig(L, "gpt2_decode_free", None, [v])
    _sig(L, "gpt2_decode_set_attn_splits", i, [v, i])
    _sig(L, "gpt2_decode_attn_splits", i, [v])
    _sig(L, "gpt2_decode_attn_waves", i, [v])
    _sig(L, "gpt2_decode_set_global_batch", i, [v, i])
    _sig(L, "gpt2_decode_global_batch", i, [v])
    _sig(L, "gpt2_decode_set_layer_kernel", i, [v, i])
    _sig(L, "gpt2_decode_fill_random_ex", i, [v, i, ctypes.c_uint64, i])
    _sig(L, "hpa_pool_fill_random_ex", i, [P, v, i, i, i, ctypes.c_uint64, i])
    _sig(L, "hpa_logits_kernel", i, [i, i, i])
    _sig(L, "gpt2_decode_layer_kernel", i, [v])
    _sig(L, "gpt2_decode_layer_plan", i, [i, i, i, i, i, i, i, i, i, _I])
    _sig(L, "gpt2_decode_set_pipe_split", i, [v, i])
    _sig(L, "hpa_decode_pipe_eligible", i, [i, i, i, i])
    _sig(L, "gpt2_decode_status", i, [v])
    _sig(L, "hpa_decode_layer_eligible", i, [i, i, i, i])
    _sig(L, "hpa_decode_layer_pick_splits", i, [i, i, i])
    _sig(L, "hpa_decode_layer_trace", i, [v, i])
    _sig(L, "hpa_decode_chain_b16_trace", i, [v, i])
    _sig(L, "hpa_decode_chain_b16_eligible", i, [i, i, i])
    _sig(L, "hpa_decode_chain_b16_eligible_cus", i, [i, i, i, i])
    _sig(L, "hpa_decode_chain_b16_sizes", i, [i, ctypes.POINTER(sz)])
    _sig(L, "hpa_decode_chain_b16", i, [ctypes.POINTER(HpaChainB16Args)])
    _sig(L, "hpa_decode_chain_b16_first", i, [ctypes.POINTER(HpaChainB16Args), v, v, v, v, sz])
    _sig(L, "hpa_decode_cx_wave_trace", i, [v])
    _sig(L, "hpa_logits_trace", i, [v])
    _sig(L, "gpt2_decode_evicted", i, [v, _I])
    _sig(L, "gpt2_decode_read_kv", i, [v, i, i, i, _F, _F])
    _sig(L, "gpt2_decode_set_kv_scales", i, [v, _F, _F])
    _sig(L, "gpt2_decode_kv_scales", i, [v, _F, _F])
    _sig(L, "gpt2_decode_batch", i, [v])
    _sig(L, "gpt2_decode_shard", i, [v, _I, i])
    _sig(L, "gpt2_decode_gather", i, [v, i])
    _sig(L, "gpt2_decode_gather_all", i, [ctypes.POINTER(v), i, i])
    _sig(L, "hpa_comm_group_start", i, [])
    _sig(L, "hpa_comm_group_end", i, [])
    _sig(L, "gpt2_decode_gather_wait", i, [v])
    _sig(L, "gpt2_decode_gathered", v, [v, i])
    _sig(L, "gpt2_decode_profile", i, [v, i])
    _sig(L, "gpt2_decode_profile_read", ctypes.c_double, [v, ctypes.POINTER(ctypes.c_long)])
    _sig(L, "hpa_frag_elems", sz, [i, i])
    _sig(L, "hpa_pack_frag", i, [v, i, i, i, v])
    _sig(L, "hpa_ln_fold_pack", i, [v, i, i, v, v, v, v, v, v])
    _sig(L, "hpa_unpack_frag", i, [v, i, i, v, i])
    _sig(L, "hpa_gemm_fused", i, [ctypes.POINTER(HpaFusedGemm)])
    _sig(L, "hpa_gemm_sk_workspace", i, [i, ctypes.POINTER(sz), ctypes.POINTER(sz)])
    _sig(L, "hpa_logits_partials", i, [ctypes.POINTER(HpaFusedGemm)])
    _sig(L, "hpa_fused_pick_waves", i, [i, i, i])
    _sig(L, "hpa_fused_pick", None, [i, i, i, _I])
    _sig(L, "hpa_fused_pick_bf16", None, [i, i, i, _I])
    _sig(L, "hpa_fused_pick_bf16_ares", i, [i, i, i, _I])
    _sig(L, "hpa_embed_frag", i, [v, v, v, v, v, v, i, i])
    _sig(L, "hpa_embed_frag_zero", i, [v, v, v, v, v, v, i, i, v, ctypes.c_size_t])
    _sig(L, "hpa_argmax_final", i, [v, i, i, i, v, v, v, v])
    _sig(L, "hpa_sample_final", i, [v, i, i, v, v, v, v, v])
    _sig(L, "hpa_sample_final_serial", i, [v, i, i, v, v, v, v, v])
    _sig(L, "hpa_sample_filtered", i, [v, i, i, v, v, v, v, v, v, v, v, v, v])
    _sig(L, "hpa_sample_filtered_ex", i, [v, i, i, v, v, v, v, v, v, v, v, v, v, v])
    _sig(L, "hpa_sample_filtered_prob", i, [v, i, i, v, v, v, v, v, v, v, v, v])
    _sig(L, "hpa_spec_accept", i, [v, v, v, v, v, v, v, i, v, v, v, v, v])
    _sig(L, "hpa_sample_filtered_prob_multi", i, [v, i, i, v, v, v, v, v, v, v, v, v, v, v])
    _sig(L, "hpa_sample_filtered_exn", i, [v, i, i, v, v, v, v, v, v, v, v, v, v, v, v])
    _sig(L, "hpa_spec_tree_accept", i, [v, v, v, v, v, v, v, v, i, v, v, v, v, v, v, v])
    _sig(L, "hpa_paged_attention_decode_frag", i, [v, P, i, v, i, v, v, i])
    _sig(L, "gpt2_decode_set_positions", i, [v, _I])
    _sig(L, "gpt2_decode_logits", v, [v])
    _sig(L, "gpt2_decode_next", v, [v])
    _sig(L, "gpt2_decode_positions", i, [v, _I])
    _sig(L, "gpt2_decode_gemm_config", i, [v, _I, _I, _I, i])
    _sig(L, "gpt2_decode_time_attention", i, [v, i, ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_double)])
    _sig(L, "gpt2_decode_time_attention_pf", i, [v, i, ctypes.c_double, i, ctypes.POINTER(ctypes.c_double),
                                                 ctypes.POINTER(ctypes.c_double)])
    _sig(L, "hpa_l3_prefetch", i, [v, sz, i])
    _sig(L, "hpa_gemm_ring_workspace", i, [i, i, ctypes.POINTER(sz), ctypes.POINTER(sz)])
    _sig(L, "gpt2_decode_step_bytes", ctypes.c_double, [v, ctypes.POINTER(ctypes.c_double)])
    _sig(L, "random_u32", ctypes.c_uint, [ctypes.POINTER(ctypes.c_ulonglong)])
    _sig(L, "random_f32", f, [ctypes.POINTER(ctypes.c_ulonglong)])
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        err = lib().hpa_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed: {err}")


def init(device=0):
    L = lib()
    if L.hpa_device_count() <= 0:
        raise RuntimeError("no HIP device visible: the MI355X path has no CPU fallback")
    check(L.hpa_init(device), "hpa_init")


def device_info():
    L = lib()
    name = ctypes.create_string_buffer(256)
    cus = ctypes.c_int()
    mem = ctypes.c_size_t()
    check(L.hpa_device_info(name, 256, ctypes.byref(cus), ctypes.byref(mem)), "device_info")
    return name.value.decode(), cus.value, mem.value


PLAN_FIELDS = ("form", "chain", "splits", "first", "attn_launch")


def layer_plan(request, B, C, num_heads, max_ctx, kv_dtype=0, w_bf16=False, num_cus=256, pick_B=None):
    """what the engine makes of set_layer_kernel(request) for these shapes on a
    device of num_cus CUs (gpt2_decode_layer_plan: the one place that decides
    it; pure, needs no GPU): a dict of PLAN_FIELDS.  pick_B: the global batch
    of a shard (default: B)."""
    out = (ctypes.c_int * 5)()
    check(lib().gpt2_decode_layer_plan(int(request), int(B), int(B if pick_B is None else pick_B), int(C),
                                       int(num_heads), int(max_ctx), int(kv_dtype), int(bool(w_bf16)),
                                       int(num_cus), out), "layer_plan")
    return dict(zip(PLAN_FIELDS, out))


# ---------------------------------------------------------------- device buffers
VERIFY_MAX_ROWS = 8  # HPA_VERIFY_MAX_ROWS
TOP_LOGPROBS_MAX = 20  # HPA_TOP_LOGPROBS_MAX


def verify_plan(max_rows, kv_dtype=0, page_size=16, head_size=64, request=0):
    """the attention kernel of a verify pass (gpt2_decode_verify_plan, pure): 1
    hpa_paged_attention_verify, 0 hpa_paged_attention_prefill_ragged.  request:
    0 auto, 1 the prefill kernel, 2 the verify kernel where it applies"""
    return int(lib().gpt2_decode_verify_plan(int(max_rows), int(kv_dtype), int(page_size), int(head_size),
                                             int(request)))


SHARED_MAX_ROWS = 8  # HPA_SHARED_MAX_ROWS


def attn_shared_plan(block_table, pos, page_size, min_tiles=1, min_members=2, max_units=None):
    """gpt2_attn_shared_plan (host only, pure): which sequences stream their
    leading 64-token tiles together.  block_table [B][stride] page ids (-1: none),
    pos [B] cached tokens.  Returns (units, unit_members [max_units][8] -1 padded,
    unit_tiles [max_units], seq_skip [B]); raises on arguments the C side refuses"""
    bt = np.ascontiguousarray(np.asarray(block_table, np.int32))
    if bt.ndim != 2:
        raise ValueError("attn_shared_plan: block_table [B][stride]")
    B, stride = bt.shape
    ps = np.ascontiguousarray(np.asarray(pos, np.int32).reshape(-1))
    if ps.size != B:
        raise ValueError("attn_shared_plan: one position per table row")
    mu = max(B // 2, 1) if max_units is None else int(max_units)
    members = np.full((max(mu, 1), SHARED_MAX_ROWS), -1, np.int32)
    tiles = np.zeros(max(mu, 1), np.int32)
    skip = np.zeros(B, np.int32)
    n = lib().gpt2_attn_shared_plan(bt.ctypes.data_as(_I), int(stride), ps.ctypes.data_as(_I), int(B), int(page_size),
                                    int(min_tiles), int(min_members), mu, members.ctypes.data_as(_I),
                                    tiles.ctypes.data_as(_I), skip.ctypes.data_as(_I))
    if n < 0:
        raise RuntimeError("gpt2_attn_shared_plan: bad arguments")
    return int(n), members, tiles, skip


def ngram_draft(history, k, max_ngram=3, min_ngram=1):
    """gpt2_ngram_draft (host only): up to k tokens that followed the most
    recent earlier occurrence of the longest matching suffix of `history`
    (n-grams of max_ngram down to min_ngram tokens); [] without a match"""
    h = np.ascontiguousarray(np.asarray(history, np.int32).reshape(-1))
    out = np.zeros(max(int(k), 1), np.int32)
    n = lib().gpt2_ngram_draft(h.ctypes.data_as(_I), int(h.size), int(max_ngram), int(min_ngram), int(k),
                               out.ctypes.data_as(_I))
    return out[:n].tolist()


def ngram_draft_tree(history, max_nodes=7, depth=4, max_branches=3, max_ngram=3, min_ngram=1):
    """gpt2_ngram_draft_tree (host only): the continuations of the earlier
    occurrences of the longest matching suffixes of `history`, most recent
    first, merged into a token tree of at most max_nodes drafts, `depth` deep,
    from at most max_branches occurrences.  Returns (ids, parents) in
    Model.verify_tree's layout: draft j is node j + 1, parents[j] its parent
    node in [0, j] (0: the pending token); ([], []) without a match"""
    h = np.ascontiguousarray(np.asarray(history, np.int32).reshape(-1))
    ids = np.zeros(VERIFY_MAX_ROWS - 1, np.int32)
    par = np.zeros(VERIFY_MAX_ROWS - 1, np.int32)
    n = lib().gpt2_ngram_draft_tree(h.ctypes.data_as(_I), int(h.size), int(max_ngram), int(min_ngram), int(max_nodes),
                                    int(depth), int(max_branches), ids.ctypes.data_as(_I), par.ctypes.data_as(_I))
    return ids[:n].tolist(), par[:n].tolist()


def tree_dense_tables(trees, row0=None):
    """gpt2_tree_dense_tables (host only): the dense-route tables of a sampled
    tree pass.  trees: as Model.verify_tree_sampled; row0 [B]: every sequence's
    first packed row (default: the rows packed in sequence order).  Returns
    (rows, seq, targets, n_targets, dst) for the NI internal nodes: targets and
    dst are (NI, VERIFY_MAX_ROWS - 1), unused entries -1"""
    B, NT = len(trees), VERIFY_MAX_ROWS - 1
    nd = np.array([-1 if t is None else len(t[0]) for t in trees], np.int32)
    live = [t for t in trees if t is not None and len(t[0])]
    cat = lambda k: np.ascontiguousarray(  # noqa: E731
        np.concatenate([np.asarray(t[k], np.int32).reshape(-1) for t in live]) if live else np.zeros(1, np.int32),
        np.int32)
    flat, par = cat(0), cat(1)
    if row0 is None:
        row0 = np.cumsum(nd + 1) - (nd + 1)
    row0 = np.ascontiguousarray(row0, np.int32)
    ND = max(int(np.maximum(nd, 0).sum()), 1)
    rows, seq, nt = (np.full(ND, -1, np.int32) for _ in range(3))
    tg, dst = (np.full((ND, NT), -1, np.int32) for _ in range(2))
    ni = lib().gpt2_tree_dense_tables(flat.ctypes.data_as(_I), par.ctypes.data_as(_I), nd.ctypes.data_as(_I), B,
                                      row0.ctypes.data_as(_I), rows.ctypes.data_as(_I), seq.ctypes.data_as(_I),
                                      tg.ctypes.data_as(_I), nt.ctypes.data_as(_I), dst.ctypes.data_as(_I))
    return rows[:ni], seq[:ni], tg[:ni], nt[:ni], dst[:ni]


def sample_filtered_prob_multi(logits, R, V, seq, temperature, top_k, top_p, targets, n_targets, dst, n_kept, cut,
                               w_target, w_total):
    """hpa_sample_filtered_prob_multi on device pointers (None where nullable)"""
    check(lib().hpa_sample_filtered_prob_multi(logits, int(R), int(V), seq, temperature, top_k, top_p, targets,
                                               n_targets, dst, n_kept, cut, w_target, w_total),
          "hpa_sample_filtered_prob_multi")


def sample_filtered_exn(logits, B, V, temperature, top_k, top_p, state, nxt, tokens, pos, active, n_kept, cut, exclude,
                        n_exclude):
    """hpa_sample_filtered_exn on device pointers (None where nullable)"""
    check(lib().hpa_sample_filtered_exn(logits, int(B), int(V), temperature, top_k, top_p, state, nxt, tokens, pos,
                                        active, n_kept, cut, exclude, n_exclude), "hpa_sample_filtered_exn")


def spec_tree_accept(w_target, w_total, drafts, parents, draft0, start, row0, lens, B, state, n_accepted, path,
                     cont_row, exclude, n_exclude, pos):
    """hpa_spec_tree_accept on device pointers"""
    check(lib().hpa_spec_tree_accept(w_target, w_total, drafts, parents, draft0, start, row0, lens, int(B), state,
                                     n_accepted, path, cont_row, exclude, n_exclude, pos), "hpa_spec_tree_accept")


class DeviceBuffer:
    """hpa_malloc'd memory with numpy-typed upload/download helpers."""

    def __init__(self, nbytes, managed=False):
        L = lib()
        self.nbytes = int(nbytes)
        self.ptr = L.hpa_malloc_managed(self.nbytes) if managed else L.hpa_malloc(self.nbytes)
        if not self.ptr:
            raise MemoryError(f"device allocation of {nbytes} bytes failed")

    @classmethod
    def from_array(cls, a, managed=False):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes, managed)
        b.upload(a)
        return b

    def upload(self, a, offset=0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        check(lib().hpa_memcpy(self.ptr + offset, a.ctypes.data, a.nbytes), "upload")

    def download(self, shape, dtype=np.float32, offset=0):
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        check(lib().hpa_memcpy(out.ctypes.data, self.ptr + offset, out.nbytes), "download")
        return out

    def free(self):
        if self.ptr:
            lib().hpa_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def to_bf16_bits(a):
    """fp32 -> bf16 bit patterns, round to nearest even (hpa::f32_to_bf16)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u.astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(a):
    """the fp32 value a bf16 KV pool stores for `a`"""
    return from_bf16_bits(to_bf16_bits(a))


# fp8 KV storage (HPA_FP8): OCP e4m3fn -- 1 sign, 4 exponent (bias 7), 3
# mantissa bits; max 448, no infinities, NaN = 0x7f / 0xff, subnormals m * 2^-9
# (the encoding of torch.float8_e4m3fn, not the MI300 fnuz form).  numpy only.
def to_fp8_bits(a):
    """fp32 -> e4m3fn codes: round to nearest even of clamp(a, -448, 448);
    NaN -> sign | 0x7f (hpa::f32_to_e4m3 at inv = 1)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    sign = ((u >> 24) & 0x80).astype(np.uint8)
    mag = u & np.uint32(0x7FFFFFFF)
    nan = mag > 0x7F800000
    mag = np.minimum(mag, np.uint32(0x43E00000))  # |x| <= 448: overflow saturates
    # normal results (|x| >= 2^-6): keep 3 mantissa bits, ties to even, rebias 127 -> 7
    norm = ((mag.astype(np.uint64) + 0x7FFFF + ((mag >> 20) & 1)) >> 20).astype(np.int64) - 960
    # subnormal results: multiples of 2^-9, rounded by an fp32 addition (ulp(2^14) = 2^-9)
    sub = (mag.view(np.float32) + np.float32(16384.0)).astype(np.float32).view(np.uint32).astype(np.int64) - 0x46800000
    code = np.where((mag >> 23) >= 121, norm, sub)
    code = np.where(nan, 0x7F, code).astype(np.uint8)
    return code | sign


def from_fp8_bits(b):
    """e4m3fn codes -> the fp32 values they stand for (exact)"""
    b = np.asarray(b, np.uint8).astype(np.int32)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, np.ldexp(m.astype(np.float32), -9),
                   np.ldexp((1.0 + m / 8.0).astype(np.float32), e - 7)).astype(np.float32)
    mag = np.where((e == 15) & (m == 7), np.float32(np.nan), mag)
    return np.where(b & 0x80, -mag, mag).astype(np.float32)


def round_fp8(a, scale=1.0):
    """the fp32 value an fp8 KV pool holds for `a` under `scale` (broadcast
    against a): decode(code(a * inv)) * scale with inv = fp32(1 / scale), every
    product an fp32 product (hip_paged_attn.h)"""
    scale = np.asarray(scale, np.float32)
    inv = (np.float32(1.0) / scale).astype(np.float32)
    a = np.asarray(a, np.float32)
    return (from_fp8_bits(to_fp8_bits((a * inv).astype(np.float32))) * scale).astype(np.float32)


HPA_F32, HPA_BF16, HPA_FP8 = 0, 1, 2


class Pool:
    """HpaKVPool: the HBM page pool in the fast layout (fp32, bf16 or fp8)."""

    def __init__(self, num_layers, num_heads, page_size, num_pages, head_size=64, managed=False, dtype=HPA_F32):
        self.s = HpaKVPool()
        check(lib().hpa_pool_create(ctypes.byref(self.s), num_layers, num_heads, head_size, page_size,
                                    num_pages, int(dtype), int(managed)), "pool_create")
        # fp8 pools: host copy of the per-head scales, (L, NH) each
        self.k_scale = np.ones((num_layers, num_heads), np.float32)
        self.v_scale = np.ones((num_layers, num_heads), np.float32)

    @property
    def ref(self):
        return ctypes.byref(self.s)

    def _k_chunk(self):
        return {HPA_BF16: 8, HPA_FP8: 16}.get(self.s.dtype, 4)

    def set_scales(self, k_scale, v_scale):
        """fp8 pools: per-head scales of K and V, (L, NH) each (or scalars),
        finite and > 0; set them before anything is written"""
        shape = (self.s.num_layers, self.s.num_heads)
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(k_scale, np.float32), shape))
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(v_scale, np.float32), shape))
        check(lib().hpa_pool_set_scales(self.ref, k.ctypes.data_as(_F), v.ctypes.data_as(_F)), "pool_set_scales")
        self.k_scale, self.v_scale = k, v

    def write_tokens(self, layer, pages, k, v):
        """host helper: k, v (ntok, C) -> logical positions 0..ntok-1 of the
        sequence whose page list is `pages` (uploads whole pages; bf16 pools
        store the round-to-nearest-even values, fp8 pools the e4m3fn codes of
        the values over the head's scale)."""
        s = self.s
        P, NH, HS, ch = s.page_size, s.num_heads, s.head_size, self._k_chunk()
        bf, f8 = s.dtype == HPA_BF16, s.dtype == HPA_FP8
        if f8:
            one = np.float32(1.0)
            k_inv = (one / self.k_scale[layer]).astype(np.float32)
            v_inv = (one / self.v_scale[layer]).astype(np.float32)
        ntok = k.shape[0]
        for lp, page in enumerate(pages):
            t0 = lp * P
            if t0 >= ntok:
                break
            n = min(P, ntok - t0)
            kt = np.zeros((NH, HS // ch, P, ch), np.float32)
            vt = np.zeros((NH, P, HS), np.float32)
            kt[:, :, :n, :] = k[t0:t0 + n].reshape(n, NH, HS // ch, ch).transpose(1, 2, 0, 3)
            vt[:, :n, :] = v[t0:t0 + n].reshape(n, NH, HS).transpose(1, 0, 2)
            if bf:
                kt, vt = to_bf16_bits(kt), to_bf16_bits(vt)
            if f8:
                kt = to_fp8_bits(kt * k_inv[:, None, None, None])
                vt = to_fp8_bits(vt * v_inv[:, None, None])
            page_k = lib().hpa_pool_tile(self.ref, layer, int(page), 0, 0)
            page_v = lib().hpa_pool_tile(self.ref, layer, int(page), 1, 0)
            check(lib().hpa_memcpy(page_k, kt.ctypes.data, kt.nbytes), "pool write K")
            check(lib().hpa_memcpy(page_v, vt.ctypes.data, vt.nbytes), "pool write V")

    def read_tokens(self, layer, pages, ntok):
        s = self.s
        P, NH, HS, ch = s.page_size, s.num_heads, s.head_size, self._k_chunk()
        bf, f8 = s.dtype == HPA_BF16, s.dtype == HPA_FP8
        et = np.uint16 if bf else np.uint8 if f8 else np.float32
        k = np.zeros((ntok, NH * HS), np.float32)
        v = np.zeros((ntok, NH * HS), np.float32)
        for lp, page in enumerate(pages):
            t0 = lp * P
            if t0 >= ntok:
                break
            n = min(P, ntok - t0)
            kt = np.empty((NH, HS // ch, P, ch), et)
            vt = np.empty((NH, P, HS), et)
            check(lib().hpa_memcpy(kt.ctypes.data, lib().hpa_pool_tile(self.ref, layer, int(page), 0, 0),
                                   kt.nbytes), "pool read K")
            check(lib().hpa_memcpy(vt.ctypes.data, lib().hpa_pool_tile(self.ref, layer, int(page), 1, 0),
                                   vt.nbytes), "pool read V")
            if bf:
                kt, vt = from_bf16_bits(kt), from_bf16_bits(vt)
            if f8:
                kt = from_fp8_bits(kt) * self.k_scale[layer][:, None, None, None]
                vt = from_fp8_bits(vt) * self.v_scale[layer][:, None, None]
            k[t0:t0 + n] = kt[:, :, :n, :].transpose(2, 0, 1, 3).reshape(n, NH * HS)
            v[t0:t0 + n] = vt[:, :n, :].transpose(1, 0, 2).reshape(n, NH * HS)
        return k, v

    def copy_pages(self, src, dst):
        """hpa_pool_copy_pages: page src[i] -> page dst[i] in every layer, one
        asynchronous launch (1..HPA_COPY_MAX_PAGES pairs of pool slots)"""
        s = np.ascontiguousarray(src, np.int32).reshape(-1)
        d = np.ascontiguousarray(dst, np.int32).reshape(-1)
        if s.size != d.size:
            raise ValueError("copy_pages: src and dst differ in length")
        check(lib().hpa_pool_copy_pages(self.ref, s.ctypes.data_as(_I), d.ctypes.data_as(_I), int(s.size)),
              "pool_copy_pages")

    def park_bytes(self, n_pages):
        """hpa_park_bytes: bytes of a parked buffer of n_pages pages (every layer)"""
        return park_bytes(self.s, n_pages)

    def park_offset(self, n_pages, layer, i):
        """hpa_park_offset: where page i of `layer` sits in a parked buffer of n_pages pages"""
        return park_offset(self.s, n_pages, layer, i)

    def gather_pages(self, pages, dst):
        """hpa_pool_gather_pages: the pages (pool slots) of every layer -> the
        contiguous buffer at `dst` (a device or pinned-host address, or an
        object with .ptr), park_bytes(len(pages)) bytes; asynchronous"""
        s = np.ascontiguousarray(pages, np.int32).reshape(-1)
        check(lib().hpa_pool_gather_pages(self.ref, s.ctypes.data_as(_I), int(s.size), getattr(dst, "ptr", dst)),
              "pool_gather_pages")

    def scatter_pages(self, pages, src):
        """hpa_pool_scatter_pages: the buffer at `src` -> the pages (distinct
        pool slots) of every layer; asynchronous"""
        s = np.ascontiguousarray(pages, np.int32).reshape(-1)
        check(lib().hpa_pool_scatter_pages(self.ref, s.ctypes.data_as(_I), int(s.size), getattr(src, "ptr", src)),
              "pool_scatter_pages")

    def destroy(self):
        if self.s.base:
            lib().hpa_pool_destroy(self.ref)

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def park_bytes(pool, n_pages):
    """hpa_park_bytes (pure: the pool's shape only; `pool` an HpaKVPool or a Pool)"""
    return int(lib().hpa_park_bytes(ctypes.byref(getattr(pool, "s", pool)), int(n_pages)))


def park_offset(pool, n_pages, layer, i):
    """hpa_park_offset (pure): byte offset of page i of `layer` in a parked buffer"""
    return int(lib().hpa_park_offset(ctypes.byref(getattr(pool, "s", pool)), int(n_pages), int(layer), int(i)))


class PinnedBuffer:
    """hpa_host_alloc'd (pinned, device-accessible) host memory; .array is a
    uint8 numpy view of it"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().hpa_host_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError(f"pinned allocation of {nbytes} bytes failed")
        self.array = np.ctypeslib.as_array((ctypes.c_ubyte * max(self.nbytes, 1)).from_address(self.ptr))[:self.nbytes]

    def free(self):
        if self.ptr:
            self.array = None
            lib().hpa_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Parked:
    """a parked sequence (GPT2Parked): host memory only; Model.unpark does not
    consume it"""

    def __init__(self, h):
        self.h = h

    @property
    def tokens(self):
        return int(lib().gpt2_parked_tokens(self.h))

    @property
    def bytes(self):
        return int(lib().gpt2_parked_bytes(self.h))

    def free(self):
        if self.h:
            lib().gpt2_parked_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------- on-disk formats
def read_checkpoint(path):
    """gpt2_read_checkpoint (host only): (GPT2Config, fp32 params in
    ParameterTensors order) from a v1 or v2 checkpoint"""
    c = GPT2Config()
    check(lib().gpt2_read_checkpoint(str(path).encode(), ctypes.byref(c), None), "read_checkpoint header")
    p = np.empty(lib().gpt2_num_parameters(c), np.float32)
    check(lib().gpt2_read_checkpoint(str(path).encode(), ctypes.byref(c), p.ctypes.data_as(_F)), "read_checkpoint")
    return c, p


def write_checkpoint(path, c, params, version=1):
    p = np.ascontiguousarray(params, np.float32)
    check(lib().gpt2_write_checkpoint_ex(str(path).encode(), c, p.ctypes.data_as(_F), int(version)),
          "write_checkpoint")


class Tokenizer(ctypes.Structure):
    """paged_infer.c:852-856"""
    _fields_ = [("vocab_size", ctypes.c_uint32), ("token_table", ctypes.POINTER(ctypes.c_char_p)),
                ("init_ok", ctypes.c_int)]

    def __init__(self, path):
        super().__init__()
        lib().tokenizer_init(ctypes.byref(self), str(path).encode())

    def decode(self, token_id):
        """the token's bytes, or None (not initialised / out of range)"""
        return lib().tokenizer_decode(ctypes.byref(self), int(token_id))

    def free(self):
        lib().tokenizer_free(ctypes.byref(self))


# ---------------------------------------------------------------- block manager
class BlockManagerStruct(ctypes.Structure):
    """include/block_manager.h BlockManager, field for field"""
    _fields_ = [("C", ctypes.c_int), ("blocks", ctypes.POINTER(KVBlock)),
                ("prompt_block_list", ctypes.POINTER(_I)), ("prompt_block_count", _I),
                ("lru_epoch", ctypes.c_int), ("max_prompts", ctypes.c_int), ("max_blocks", ctypes.c_int),
                ("block_size", ctypes.c_int), ("max_blocks_per_prompt", ctypes.c_int), ("block_table", _I),
                ("free_bits", ctypes.POINTER(ctypes.c_ulonglong)), ("free_words", ctypes.c_int),
                ("free_hint", ctypes.c_int), ("free_count", ctypes.c_int),
                ("backend_alloc", _V), ("backend_release", _V), ("backend_ctx", _V),
                ("dirty_lo", ctypes.c_int), ("dirty_hi", ctypes.c_int), ("last_evicted_prompt", ctypes.c_int),
                ("page_refs", _I), ("shared_pages", ctypes.c_int)]


class BlockManager:
    """block_manager.c API (create_block_manager, request_block, ...)."""

    def __init__(self, channels, max_prompts=None, max_blocks=None, block_size=None,
                 max_blocks_per_prompt=None, host_pages=False):
        L = lib()
        if max_prompts is None:
            self.h = L.create_block_manager(channels)
        else:
            self.h = L.create_block_manager_ex(channels, max_prompts, max_blocks, block_size,
                                               max_blocks_per_prompt or max_blocks)
        if not self.h:
            raise MemoryError("create_block_manager failed")
        if host_pages:
            L.bm_use_host_pages(self.h)

    def request_block(self, prompt):
        blk = lib().request_block(self.h, prompt)
        return lib().bm_block_index(self.h, blk) if blk else -1

    def block(self, index):
        base = ctypes.cast(self.h, ctypes.POINTER(ctypes.c_void_p))
        blocks = ctypes.cast(base[1], ctypes.POINTER(KVBlock))  # BlockManager.blocks
        return blocks[index]

    def fork(self, src, dst, n_pages):
        """bm_fork_prompt: dst (owning no pages) shares src's first n_pages
        pages; raises on a bad argument (nothing changed then)"""
        if lib().bm_fork_prompt(self.h, int(src), int(dst), int(n_pages)) != 0:
            raise ValueError(f"bm_fork_prompt({src}, {dst}, {n_pages}) refused")

    def refs(self, page):
        """holders of a page (0 = free)"""
        return lib().bm_page_refs(self.h, int(page))

    def shared_pages(self):
        """pages with more than one holder"""
        return lib().bm_shared_pages(self.h)

    def free_pages(self):
        return lib().bm_free_pages(self.h)

    def free_prompt(self, prompt):
        lib().free_blocks_for_prompt(self.h, int(prompt))

    def struct(self):
        """the C struct (fields of include/block_manager.h)"""
        return ctypes.cast(self.h, ctypes.POINTER(BlockManagerStruct)).contents

    def pages(self, prompt):
        """the prompt's page list"""
        bm = self.struct()
        return [bm.prompt_block_list[prompt][i] for i in range(bm.prompt_block_count[prompt])]

    def last_evicted(self):
        """the prompt the last request_block paged out, or -1"""
        return self.struct().last_evicted_prompt

    def close(self):
        if self.h:
            lib().destroy_block_manager(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- model / decode engine
class Model:
    """GPT2 + the decode engine (gpt2_decode_*), i.e. the hot path."""

    def __init__(self, cfg, params=None, seed=1337, checkpoint=None):
        L = lib()
        if checkpoint is not None:  # config from the file's header
            cfg = GPT2Config()
            check(L.gpt2_read_checkpoint(str(checkpoint).encode(), ctypes.byref(cfg), None), "checkpoint header")
        self.cfg = cfg if isinstance(cfg, GPT2Config) else config(cfg)
        self.h = L.gpt2_alloc()
        if checkpoint is not None:
            L.gpt2_build_from_checkpoint(self.h, str(checkpoint).encode())
        elif params is not None:
            p = np.ascontiguousarray(params, np.float32)
            assert p.size == L.gpt2_num_parameters(self.cfg)
            check(L.gpt2_build_from_params(self.h, self.cfg, p.ctypes.data_as(_F)), "build_from_params")
        else:
            check(L.gpt2_build_synthetic(self.h, self.cfg, seed), "build_synthetic")
        self.B = 0

    def set_manager(self, bm):
        """model.manager = bm (paged_infer.c:986-987): the engine's pages come
        from this manager's capacity, with its LRU policy"""
        self._bm = bm
        lib().gpt2_set_manager(self.h, bm.h)

    def decode_init(self, B, page_size=16, max_ctx=None, kv_dtype=HPA_F32, w_dtype=HPA_F32):
        max_ctx = max_ctx or self.cfg.max_seq_len
        check(lib().gpt2_decode_init_w(self.h, B, page_size, max_ctx, int(kv_dtype), int(w_dtype)),
              "gpt2_decode_init")
        self.B = B

    def set_graph(self, on):
        check(lib().gpt2_decode_set_graph(self.h, int(on)), "set_graph")

    def step(self, tokens=None, want_next=True):
        nxt = np.zeros(self.B, np.int32) if want_next else None
        tp = None
        if tokens is not None:
            tokens = np.ascontiguousarray(tokens, np.int32)
            assert tokens.shape == (self.B,)
            tp = tokens.ctypes.data_as(_I)
        check(lib().gpt2_decode_step(self.h, tp, nxt.ctypes.data_as(_I) if want_next else None),
              "gpt2_decode_step")
        return nxt

    def step_traced(self, tokens=None):
        """one eager step; returns (next ids, the residual stream entering every
        layer and the final one, (L+1, B, C))"""
        nxt = np.zeros(self.B, np.int32)
        xs = np.zeros((self.cfg.num_layers + 1, self.B, self.cfg.channels), np.float32)
        tp = None
        if tokens is not None:
            tokens = np.ascontiguousarray(tokens, np.int32)
            tp = tokens.ctypes.data_as(_I)
        check(lib().gpt2_decode_step_traced(self.h, tp, nxt.ctypes.data_as(_I), xs.ctypes.data_as(_F)),
              "gpt2_decode_step_traced")
        return nxt, xs

    def trace_next_pass(self, rows, floats=None):
        """gpt2_decode_trace_next_pass: arms the next dense pass (prefill,
        prefill_ragged, score, score_top, verify) and that one only.  Returns
        the array the pass fills, (L+1, rows, C) float32: the residual stream
        after the embedding and after every layer, rows in the pass's packed
        order.  rows must be at least the pass's row count (a verify pass of
        n drafts has n + 1 rows per live sequence); the first R of them are
        written when it is more -- then as a flat [L+1][R][C] block at the
        start of the array -- and a pass that needs more is refused.  floats
        overrides the room the engine is told of (tests of that refusal).
        The engine writes into the array's memory during the pass, so the
        model keeps a reference to it until the next call of this method."""
        xs = np.zeros((self.cfg.num_layers + 1, int(rows), self.cfg.channels), np.float32)
        self._trace_xs = xs  # a caller that drops the result must not leave the engine a dangling pointer
        check(lib().gpt2_decode_trace_next_pass(self.h, xs.ctypes.data_as(_F), xs.size if floats is None else int(floats)),
              "gpt2_decode_trace_next_pass")
        return xs

    def step_async(self, tokens=None):
        tp = None
        if tokens is not None:
            tokens = np.ascontiguousarray(tokens, np.int32)
            tp = tokens.ctypes.data_as(_I)
        check(lib().gpt2_decode_step_async(self.h, tp), "gpt2_decode_step_async")

    def logits(self):
        ptr = lib().gpt2_decode_logits(self.h)
        out = np.empty((self.B, self.cfg.vocab_size), np.float32)
        check(lib().hpa_memcpy(out.ctypes.data, ptr, out.nbytes), "logits download")
        return out

    def logits_ptr(self):
        return lib().gpt2_decode_logits(self.h)

    def next_ptr(self):
        return lib().gpt2_decode_next(self.h)

    def positions(self):
        out = np.zeros(self.B, np.int32)
        check(lib().gpt2_decode_positions(self.h, out.ctypes.data_as(_I)), "positions")
        return out

    def set_attn_splits(self, splits):
        """context ranges per (sequence, head) of the decode attention (0 = by shape)"""
        check(lib().gpt2_decode_set_attn_splits(self.h, int(splits)), "set_attn_splits")
        return lib().gpt2_decode_attn_splits(self.h)

    def attn_splits(self):
        return lib().gpt2_decode_attn_splits(self.h)

    def attn_waves(self):
        return lib().gpt2_decode_attn_waves(self.h)

    def set_global_batch(self, total):
        """shape picks of the unsharded engine of `total` rows (<= 64; 0 = this
        engine's own B): a shard's rows then equal that engine's bit for bit"""
        check(lib().gpt2_decode_set_global_batch(self.h, int(total)), "set_global_batch")

    def set_layer_kernel(self, on):
        """the layer loop's form, a request 0..7: 0 five launches, 1 the form
        measured fastest for the shape, 2 full persistent layer, 3 attention
        launch + chain of 4-wave units, 4 the chain with wide units, 5 chain
        form 6 (12-wave multi-tile units, C = 768), 6 chain form 8 (streamed
        weights, C = 768 .. 1600), 7 the pipelined halves (else 5); 2, 4 and
        7 in A/B builds only (bf16 weights: any nonzero value is the bf16
        chain, B <= 256).  What a request becomes for a shape is decided by
        layer_plan() (gpt2_decode_layer_plan, include/paged_infer.h) alone;
        returns whether a persistent form is now in use"""
        check(lib().gpt2_decode_set_layer_kernel(self.h, int(on)), "set_layer_kernel")
        return bool(lib().gpt2_decode_layer_kernel(self.h))

    def layer_kernel(self):
        return bool(lib().gpt2_decode_layer_kernel(self.h))

    def set_pipe_split(self, g_cus):
        """CUs of the pipelined halves' GEMM role (form 7; multiple of 8, 0 = 64)"""
        check(lib().gpt2_decode_set_pipe_split(self.h, int(g_cus)), "set_pipe_split")

    def layer_form(self):
        """the plan's form (layer_plan): 0 five launches per layer, 1 full persistent layer,
        2 attention launch + chain of 4-wave units, 3 attention launch + the chain in wide /
        multi-tile / streamed-weight units, 4 the bf16-weight chain (hpa_chain_b16.hip),
        5 the pipelined halves (hpa_pipe.hip)"""
        return int(lib().gpt2_decode_layer_kernel(self.h))

    def status(self):
        """waits for queued work; raises if a persistent-layer wait timed out"""
        code = lib().gpt2_decode_status(self.h)
        if code:
            raise RuntimeError(f"decode step failed (status {code})")

    def evicted(self):
        """sequences the LRU policy paged out since the last call (bool mask)"""
        m = np.zeros(self.B, np.int32)
        n = lib().gpt2_decode_evicted(self.h, m.ctypes.data_as(_I))
        if n < 0:
            raise RuntimeError("evicted: no engine")
        return m.astype(bool)

    def read_kv(self, layer, b, n):
        """K, V of positions [0, n) of sequence b, token-major (n, C) fp32"""
        C = self.cfg.channels
        k = np.zeros((n, C), np.float32)
        v = np.zeros((n, C), np.float32)
        check(lib().gpt2_decode_read_kv(self.h, int(layer), int(b), int(n), k.ctypes.data_as(_F),
                                        v.ctypes.data_as(_F)), "read_kv")
        return k, v

    def set_kv_scales(self, k_scale, v_scale):
        """fp8 KV pool: per-head scales of K and V, (L, NH) each (or scalars),
        finite and > 0; only while every sequence is at position 0"""
        shape = (self.cfg.num_layers, self.cfg.num_heads)
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(k_scale, np.float32), shape))
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(v_scale, np.float32), shape))
        check(lib().gpt2_decode_set_kv_scales(self.h, k.ctypes.data_as(_F), v.ctypes.data_as(_F)), "set_kv_scales")

    def kv_scales(self):
        """fp8 KV pool: (k_scale, v_scale), (L, NH) each"""
        shape = (self.cfg.num_layers, self.cfg.num_heads)
        k, v = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        check(lib().gpt2_decode_kv_scales(self.h, k.ctypes.data_as(_F), v.ctypes.data_as(_F)), "kv_scales")
        return k, v

    def shard(self, rows_per_rank, root=0):
        """sequence-sharded decode: this rank's row count among rows_per_rank
        (after hpa_comm_init); gather() then runs the RCCL end-of-step gather"""
        r = np.ascontiguousarray(rows_per_rank, np.int32)
        check(lib().gpt2_decode_shard(self.h, r.ctypes.data_as(_I), int(root)), "shard")

    def gather(self, what=0):
        check(lib().gpt2_decode_gather(self.h, int(what)), "gather")

    def gathered(self, total_rows, what=0):
        """root: host copy of the last gather (waits for it)"""
        check(lib().gpt2_decode_gather_wait(self.h), "gather_wait")
        ptr = lib().gpt2_decode_gathered(self.h, int(what))
        if not ptr:
            return None
        out = np.empty((total_rows, self.cfg.vocab_size) if what == 0 else (total_rows,),
                       np.float32 if what == 0 else np.int32)
        check(lib().hpa_memcpy(out.ctypes.data, ptr, out.nbytes), "gathered download")
        return out

    def time_attention(self, iters=48):
        """(avg ms, algorithmic bytes) per launch of the decode attention
        kernel, back-to-back launches at the last step's positions"""
        ms, by = ctypes.c_double(), ctypes.c_double()
        check(lib().gpt2_decode_time_attention(self.h, int(iters), ctypes.byref(ms), ctypes.byref(by)),
              "time_attention")
        return ms.value, by.value

    def time_attention_pf(self, frac, iters=24, grid=1024):
        """(attention ms, prefetch ms) per iteration: the first `frac` of the
        layer's pool slab read into the Infinity Cache, then its attention"""
        a, p = ctypes.c_double(), ctypes.c_double()
        check(lib().gpt2_decode_time_attention_pf(self.h, int(iters), float(frac), int(grid), ctypes.byref(a),
                                                  ctypes.byref(p)), "time_attention_pf")
        return a.value, p.value

    def prefill(self, tokens):
        """tokens (B, T): all T tokens of every sequence in one pass; returns
        the greedy next ids (B,)"""
        tokens = np.ascontiguousarray(tokens, np.int32)
        assert tokens.ndim == 2 and tokens.shape[0] == self.B
        nxt = np.zeros(self.B, np.int32)
        check(lib().gpt2_decode_prefill(self.h, tokens.ctypes.data_as(_I), tokens.shape[1],
                                        nxt.ctypes.data_as(_I)), "prefill")
        return nxt

    def prefill_ragged(self, seqs):
        """seqs: B token lists (empty = sequence untouched); one pass over
        all of them (continuous batching); returns the next ids (B,)"""
        assert len(seqs) == self.B
        lens = np.array([len(t) for t in seqs], np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32).reshape(-1) for t in seqs])
                                    if lens.sum() else np.zeros(1, np.int32), np.int32)
        nxt = np.zeros(self.B, np.int32)
        check(lib().gpt2_decode_prefill_ragged(self.h, flat.ctypes.data_as(_I), lens.ctypes.data_as(_I),
                                               nxt.ctypes.data_as(_I)), "prefill_ragged")
        return nxt

    def score(self, seqs, targets=None):
        """gpt2_decode_score: prefill_ragged(seqs) that also returns every
        token's log-probability.  targets: per sequence, the id whose
        log-probability each position reports (-1: none, 0.0 returned);
        None shifts: the target of token t is token t + 1 and the last token
        has none, so len(seq) - 1 values are meaningful.  Returns (logprobs,
        top_ids, next_ids): per-sequence float32 / int32 arrays of len(seq)
        (top_ids: each position's greedy id) and the next ids (B,)."""
        assert len(seqs) == self.B
        seqs = [np.asarray(t, np.int32).reshape(-1) for t in seqs]
        if targets is None:
            targets = [np.concatenate([t[1:], np.full(1, -1, np.int32)]) if len(t) else t for t in seqs]
        targets = [np.asarray(t, np.int32).reshape(-1) for t in targets]
        assert len(targets) == self.B and all(len(a) == len(b) for a, b in zip(seqs, targets))
        lens = np.array([len(t) for t in seqs], np.int32)
        R = int(lens.sum())
        flat = np.ascontiguousarray(np.concatenate(seqs) if R else np.zeros(1, np.int32), np.int32)
        tgt = np.ascontiguousarray(np.concatenate(targets) if R else np.full(1, -1, np.int32), np.int32)
        lp = np.zeros(max(R, 1), np.float32)
        top = np.zeros(max(R, 1), np.int32)
        nxt = np.zeros(self.B, np.int32)
        check(lib().gpt2_decode_score(self.h, flat.ctypes.data_as(_I), lens.ctypes.data_as(_I), tgt.ctypes.data_as(_I),
                                      lp.ctypes.data_as(_F), top.ctypes.data_as(_I), nxt.ctypes.data_as(_I)), "score")
        cuts = np.cumsum(lens)[:-1]
        return np.split(lp[:R], cuts), np.split(top[:R], cuts), nxt

    def verify(self, drafts, want_logprobs=False):
        """gpt2_decode_verify: one speculative greedy pass.  drafts: per
        sequence a list of up to VERIFY_MAX_ROWS - 1 drafted ids ([]: a plain
        decode step of that sequence) or None (sequence untouched).  Returns
        (n_accepted, tokens, logprobs), per-sequence lists with None for an
        untouched sequence: tokens[b] = the accepted drafts and then the
        model's own next token (n_accepted[b] + 1 ids); logprobs[b] (None
        unless want_logprobs) = log p(draft i | pending id, drafts before it)
        for every drafted id, accepted or not."""
        assert len(drafts) == self.B
        nd = np.array([-1 if t is None else len(t) for t in drafts], np.int32)
        parts = [np.asarray(t, np.int32).reshape(-1) for t in drafts if t is not None and len(t)]
        flat = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(1, np.int32), np.int32)
        acc = np.zeros(self.B, np.int32)
        toks = np.zeros((self.B, VERIFY_MAX_ROWS), np.int32)
        lp = np.zeros((self.B, VERIFY_MAX_ROWS), np.float32)
        check(lib().gpt2_decode_verify(self.h, flat.ctypes.data_as(_I), nd.ctypes.data_as(_I), acc.ctypes.data_as(_I),
                                       toks.ctypes.data_as(_I), lp.ctypes.data_as(_F) if want_logprobs else None),
              "verify")
        live = [int(n) >= 0 for n in nd]
        return ([int(acc[b]) if live[b] else None for b in range(self.B)],
                [toks[b, :acc[b] + 1].tolist() if live[b] else None for b in range(self.B)],
                [lp[b, :nd[b]].copy() if live[b] and want_logprobs else None for b in range(self.B)])

    def verify_tree(self, trees):
        """gpt2_decode_verify_tree: one speculative greedy pass over a draft
        tree per sequence.  trees[b]: None (sequence untouched) or (ids,
        parents), up to VERIFY_MAX_ROWS - 1 drafted ids with parents[j] in
        [0, j] the node draft j hangs from (node 0: the pending id; draft j is
        node j + 1; ([], []) is a plain decode step).  Returns (n_accepted,
        tokens, nodes), per-sequence lists with None for an untouched sequence:
        tokens[b] = the accepted drafts along the path and then the model's own
        next token; nodes[b] = the accepted drafts' node indices."""
        assert len(trees) == self.B
        nd = np.array([-1 if t is None else len(t[0]) for t in trees], np.int32)
        assert all(t is None or len(t[0]) == len(t[1]) for t in trees)
        live_parts = [t for t in trees if t is not None and len(t[0])]
        cat = lambda k: np.ascontiguousarray(  # noqa: E731
            np.concatenate([np.asarray(t[k], np.int32).reshape(-1) for t in live_parts]) if live_parts
            else np.zeros(1, np.int32), np.int32)
        flat, par = cat(0), cat(1)
        acc = np.zeros(self.B, np.int32)
        toks = np.zeros((self.B, VERIFY_MAX_ROWS), np.int32)
        nodes = np.zeros((self.B, VERIFY_MAX_ROWS), np.int32)
        check(lib().gpt2_decode_verify_tree(self.h, flat.ctypes.data_as(_I), par.ctypes.data_as(_I),
                                            nd.ctypes.data_as(_I), acc.ctypes.data_as(_I), toks.ctypes.data_as(_I),
                                            nodes.ctypes.data_as(_I)), "verify_tree")
        live = [int(n) >= 0 for n in nd]
        return ([int(acc[b]) if live[b] else None for b in range(self.B)],
                [toks[b, :acc[b] + 1].tolist() if live[b] else None for b in range(self.B)],
                [nodes[b, :acc[b]].tolist() if live[b] else None for b in range(self.B)])

    def verify_tree_sampled(self, trees, want_probs=False):
        """gpt2_decode_verify_tree_sampled: verify_tree under sampling mode 2
        (multi-draft rejection sampling over point-mass siblings, exact).
        Arguments and the first three results as verify_tree(); with
        want_probs a fourth, probs[b] = the mass mode 2 gives every drafted id
        at its parent's row, examined or not."""
        assert len(trees) == self.B
        nd = np.array([-1 if t is None else len(t[0]) for t in trees], np.int32)
        assert all(t is None or len(t[0]) == len(t[1]) for t in trees)
        live_parts = [t for t in trees if t is not None and len(t[0])]
        cat = lambda k: np.ascontiguousarray(  # noqa: E731
            np.concatenate([np.asarray(t[k], np.int32).reshape(-1) for t in live_parts]) if live_parts
            else np.zeros(1, np.int32), np.int32)
        flat, par = cat(0), cat(1)
        acc = np.zeros(self.B, np.int32)
        toks = np.zeros((self.B, VERIFY_MAX_ROWS), np.int32)
        nodes = np.zeros((self.B, VERIFY_MAX_ROWS), np.int32)
        pr = np.zeros((self.B, VERIFY_MAX_ROWS), np.float32)
        check(lib().gpt2_decode_verify_tree_sampled(self.h, flat.ctypes.data_as(_I), par.ctypes.data_as(_I),
                                                    nd.ctypes.data_as(_I), acc.ctypes.data_as(_I),
                                                    toks.ctypes.data_as(_I), nodes.ctypes.data_as(_I),
                                                    pr.ctypes.data_as(_F) if want_probs else None),
              "verify_tree_sampled")
        live = [int(n) >= 0 for n in nd]
        out = ([int(acc[b]) if live[b] else None for b in range(self.B)],
               [toks[b, :acc[b] + 1].tolist() if live[b] else None for b in range(self.B)],
               [nodes[b, :acc[b]].tolist() if live[b] else None for b in range(self.B)])
        if want_probs:
            out += ([pr[b, :nd[b]].copy() if live[b] else None for b in range(self.B)],)
        return out

    def verify_sampled(self, drafts, want_probs=False):
        """gpt2_decode_verify_sampled: one speculative pass under sampling
        mode 2 (per-sequence temperature / top-k / top-p), drafts as point-mass
        proposals.  Arguments and the first two results as verify(); the third,
        probs[b] (None unless want_probs), = the mass mode 2 gives every
        drafted id at its row, examined or not."""
        assert len(drafts) == self.B
        nd = np.array([-1 if t is None else len(t) for t in drafts], np.int32)
        parts = [np.asarray(t, np.int32).reshape(-1) for t in drafts if t is not None and len(t)]
        flat = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(1, np.int32), np.int32)
        acc = np.zeros(self.B, np.int32)
        toks = np.zeros((self.B, VERIFY_MAX_ROWS), np.int32)
        pr = np.zeros((self.B, VERIFY_MAX_ROWS), np.float32)
        check(lib().gpt2_decode_verify_sampled(self.h, flat.ctypes.data_as(_I), nd.ctypes.data_as(_I),
                                               acc.ctypes.data_as(_I), toks.ctypes.data_as(_I),
                                               pr.ctypes.data_as(_F) if want_probs else None), "verify_sampled")
        live = [int(n) >= 0 for n in nd]
        return ([int(acc[b]) if live[b] else None for b in range(self.B)],
                [toks[b, :acc[b] + 1].tolist() if live[b] else None for b in range(self.B)],
                [pr[b, :nd[b]].copy() if live[b] and want_probs else None for b in range(self.B)])

    def set_verify_attention(self, request=0):
        """the attention kernel of verify(): 0 auto, 1 the prefill kernel, 2 the
        few-row verify kernel where it applies (verify_plan)"""
        check(lib().gpt2_decode_set_verify_attention(self.h, int(request)), "set_verify_attention")

    def set_score_chunk(self, rows=0):
        """rows per SCORE GEMM of score(): 0 = the default, else a positive
        multiple of 16"""
        check(lib().gpt2_decode_set_score_chunk(self.h, int(rows)), "set_score_chunk")

    def set_logprobs(self, enable=True):
        """after every pick also compute the chosen id's log-probability
        (raw model distribution: temperature 1, no filter); see logprobs()"""
        check(lib().gpt2_decode_set_logprobs(self.h, int(bool(enable))), "set_logprobs")

    def logprobs(self):
        """(B,) log-probabilities of the ids the last pick chose (sequences a
        ragged call left untouched keep their value); set_logprobs first"""
        out = np.zeros(self.B, np.float32)
        check(lib().gpt2_decode_logprobs(self.h, out.ctypes.data_as(_F)), "logprobs")
        return out

    def set_top_logprobs(self, k):
        """after every pick also select the k (0..TOP_LOGPROBS_MAX, 0 = off) most
        likely ids of the raw model distribution with their log-probabilities;
        see top_logprobs()"""
        check(lib().gpt2_decode_set_top_logprobs(self.h, int(k)), "set_top_logprobs")

    def top_logprobs(self):
        """(ids (B, k) int32, logprobs (B, k) float32) of the last pick's rows:
        entry j is the j-th most likely id (equal logits: the lower id first);
        sequences a ragged call left untouched keep their values;
        set_top_logprobs first"""
        k = lib().gpt2_decode_top_logprobs_k(self.h)
        if k <= 0:
            raise RuntimeError("top_logprobs: off (set_top_logprobs(k) first)")
        ids = np.zeros((self.B, k), np.int32)
        lps = np.zeros((self.B, k), np.float32)
        check(lib().gpt2_decode_top_logprobs(self.h, ids.ctypes.data_as(_I), lps.ctypes.data_as(_F)), "top_logprobs")
        return ids, lps

    def score_top(self, seqs, k, targets=None):
        """gpt2_decode_score_top: score(seqs, targets) that also returns every
        position's k most likely ids and their log-probabilities.  Returns
        (logprobs, top_ids, top_lps, next_ids): per-sequence arrays of
        len(seq), (len(seq), k) int32 and (len(seq), k) float32, and the next
        ids (B,)."""
        assert len(seqs) == self.B
        seqs = [np.asarray(t, np.int32).reshape(-1) for t in seqs]
        if targets is None:
            targets = [np.concatenate([t[1:], np.full(1, -1, np.int32)]) if len(t) else t for t in seqs]
        targets = [np.asarray(t, np.int32).reshape(-1) for t in targets]
        assert len(targets) == self.B and all(len(a) == len(b) for a, b in zip(seqs, targets))
        lens = np.array([len(t) for t in seqs], np.int32)
        R = int(lens.sum())
        k = int(k)
        flat = np.ascontiguousarray(np.concatenate(seqs) if R else np.zeros(1, np.int32), np.int32)
        tgt = np.ascontiguousarray(np.concatenate(targets) if R else np.full(1, -1, np.int32), np.int32)
        lp = np.zeros(max(R, 1), np.float32)
        ids = np.zeros((max(R, 1), max(k, 1)), np.int32)
        lps = np.zeros((max(R, 1), max(k, 1)), np.float32)
        nxt = np.zeros(self.B, np.int32)
        check(lib().gpt2_decode_score_top(self.h, flat.ctypes.data_as(_I), lens.ctypes.data_as(_I),
                                          tgt.ctypes.data_as(_I), lp.ctypes.data_as(_F), k, ids.ctypes.data_as(_I),
                                          lps.ctypes.data_as(_F), nxt.ctypes.data_as(_I)), "score_top")
        cuts = np.cumsum(lens)[:-1]
        return np.split(lp[:R], cuts), np.split(ids[:R], cuts), np.split(lps[:R], cuts), nxt

    def release(self, seq):
        """retire sequence seq: pages back to the pool, position 0"""
        check(lib().gpt2_decode_release(self.h, int(seq)), "release")

    def fork(self, src, dst, n_tokens=-1):
        """gpt2_decode_fork: slot dst (fresh or released) continues from the
        first n_tokens cached tokens of slot src (-1: all of them), sharing
        its full pages and copying only the partly filled one.  With all of
        them dst also inherits src's pending next id (step(None) continues
        both); its sampler state stays its own."""
        check(lib().gpt2_decode_fork(self.h, int(src), int(dst), int(n_tokens)), "fork")

    def park(self, seq, keep=False):
        """gpt2_decode_park: everything that belongs to sequence seq (K/V pages,
        pending id, sampler state, readback rows, settings, history) into host
        memory; the slot is released unless keep (a checkpoint).  Returns a
        Parked"""
        h = lib().gpt2_decode_park(self.h, int(seq), int(bool(keep)))
        if not h:
            raise RuntimeError(f"park({seq}) refused")
        return Parked(h)

    def unpark(self, parked, seq):
        """gpt2_decode_unpark: the parked sequence into slot seq (fresh or
        released), in private pages; step(None) continues it bit for bit.
        Raises, nothing changed, when refused (paged_infer.h)"""
        if not isinstance(parked, Parked) or not parked.h:
            raise ValueError("unpark: a live Parked handle expected")
        if lib().gpt2_decode_unpark(self.h, parked.h, int(seq)) != 0:
            raise RuntimeError(f"unpark into {seq} refused")

    def set_shared_attention(self, on=True, min_tiles=None, min_members=None, min_covered=None):
        """gpt2_decode_set_shared_attention: the decode attention streams the
        leading 64-token tiles that up to 8 forks hold in the same pages once
        per unit (fp32 pools only; raises on a bf16 / fp8 pool).  min_tiles /
        min_members / min_covered override the plan's measured thresholds
        (15 tiles, 2 members, units covering 64 sequences)."""
        if min_tiles is not None or min_members is not None or min_covered is not None:
            t, m, c = self.shared_thresholds()
            check(lib().gpt2_decode_set_shared_thresholds(self.h, int(t if min_tiles is None else min_tiles),
                                                          int(m if min_members is None else min_members),
                                                          int(c if min_covered is None else min_covered)),
                  "set_shared_thresholds")
        check(lib().gpt2_decode_set_shared_attention(self.h, int(bool(on))), "set_shared_attention")

    def shared_attention(self):
        return bool(lib().gpt2_decode_shared_attention(self.h))

    def shared_thresholds(self):
        """the plan's (min_tiles, min_members, min_covered)"""
        t, m, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        check(lib().gpt2_decode_shared_thresholds(self.h, ctypes.byref(t), ctypes.byref(m), ctypes.byref(c)),
              "shared_thresholds")
        return t.value, m.value, c.value

    def shared_plan(self):
        """gpt2_decode_shared_plan: (units, unit_of [B] (-1: none), shared_tokens [B])"""
        unit_of = np.zeros(self.B, np.int32)
        tok = np.zeros(self.B, np.int32)
        n = lib().gpt2_decode_shared_plan(self.h, unit_of.ctypes.data_as(_I), tok.ctypes.data_as(_I))
        if n < 0:
            raise RuntimeError("shared_plan: no engine")
        return int(n), unit_of, tok

    def shared_splits(self):
        """ranges per (unit, head) of the prefix launch of the plan in use"""
        return int(lib().gpt2_decode_shared_splits(self.h))

    def set_shared_splits(self, splits):
        """0: by shape (hpa_attn_shared_pick_splits), else 1..16"""
        check(lib().gpt2_decode_set_shared_splits(self.h, int(splits)), "set_shared_splits")

    def free_pages(self):
        """free pages of the engine's block manager"""
        return lib().gpt2_decode_free_pages(self.h)

    def page_slots(self, n):
        """gpt2_decode_page_slots: the pool slot of each of the manager's pages 0 .. n-1"""
        out = np.zeros(int(n), np.int32)
        got = lib().gpt2_decode_page_slots(self.h, out.ctypes.data_as(_I), int(n))
        if got < 0:
            raise RuntimeError("page_slots: no engine")
        return out[:got]

    def set_sampling(self, enable=True, seed=1337, filtered=False):
        """token choice: greedy (enable=False), the reference's multinomial
        draw, or with filtered=True temperature / top-k / top-p per sequence
        (set_sampling_params); sequence b's coins start at seed + b"""
        mode = 2 if (enable and filtered) else int(bool(enable))
        check(lib().gpt2_decode_set_sampling(self.h, mode, int(seed)), "set_sampling")

    def set_sampling_params(self, seq=-1, temperature=1.0, top_k=0, top_p=1.0):
        """filtered sampling's settings of sequence seq (-1: every sequence):
        temperature >= 0 (0 = greedy), top_k >= 0 (0 = off), 0 < top_p <= 1"""
        check(lib().gpt2_decode_set_sampling_params(self.h, int(seq), float(temperature), int(top_k),
                                                    float(top_p)), "set_sampling_params")

    def sampling_params(self, seq):
        """(temperature, top_k, top_p) of sequence seq"""
        t, k, p = ctypes.c_float(), ctypes.c_int(), ctypes.c_float()
        check(lib().gpt2_decode_sampling_params(self.h, int(seq), ctypes.byref(t), ctypes.byref(k),
                                                ctypes.byref(p)), "sampling_params")
        return t.value, k.value, p.value

    def seed_sequence(self, seq, seed):
        """restart sequence seq's coin stream at seed"""
        check(lib().gpt2_decode_seed_sequence(self.h, int(seq), int(seed)), "seed_sequence")

    def sampler_state(self, seq):
        """sequence seq's sampler state (its coin stream's position); waits for queued work"""
        st = ctypes.c_ulonglong()
        check(lib().gpt2_decode_sampler_state(self.h, int(seq), ctypes.byref(st)), "sampler_state")
        return int(st.value)

    def set_processors(self, enable=True):
        """logit processors (penalties by the fed tokens, logit bias) before
        every pick; needs every sequence at position 0 (paged_infer.h)"""
        check(lib().gpt2_decode_set_processors(self.h, int(bool(enable))), "set_processors")

    def processors(self):
        return bool(lib().gpt2_decode_processors(self.h))

    def set_penalties(self, seq=-1, repetition=1.0, presence=0.0, frequency=0.0, from_pos=0):
        """sequence seq's (-1: every sequence's) penalties over the tokens fed
        at positions >= from_pos: repetition > 0 (1 = off, HF rule), presence
        and frequency (0 = off, OpenAI rule)"""
        check(lib().gpt2_decode_set_penalties(self.h, int(seq), float(repetition), float(presence),
                                              float(frequency), int(from_pos)), "set_penalties")

    def penalties(self, seq):
        """(repetition, presence, frequency, from_pos) of sequence seq"""
        r, p, f, w = ctypes.c_float(), ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        check(lib().gpt2_decode_penalties(self.h, int(seq), ctypes.byref(r), ctypes.byref(p), ctypes.byref(f),
                                          ctypes.byref(w)), "penalties")
        return r.value, p.value, f.value, w.value

    def set_logit_bias(self, seq, ids, values):
        """replace sequence seq's (-1: every sequence's) bias list: at most
        300 distinct ids, values finite or -inf (a ban); empty lists clear it"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        values = np.ascontiguousarray(values, np.float32).reshape(-1)
        if ids.size != values.size:
            raise ValueError("set_logit_bias: ids and values differ in length")
        check(lib().gpt2_decode_set_logit_bias(self.h, int(seq), ids.ctypes.data_as(_I), values.ctypes.data_as(_F),
                                               int(ids.size)), "set_logit_bias")

    def logit_bias(self, seq):
        """(ids, values) of sequence seq's bias list"""
        ids, values, n = np.zeros(300, np.int32), np.zeros(300, np.float32), ctypes.c_int()
        check(lib().gpt2_decode_logit_bias(self.h, int(seq), ids.ctypes.data_as(_I), values.ctypes.data_as(_F),
                                           ctypes.byref(n)), "logit_bias")
        return ids[:n.value].copy(), values[:n.value].copy()

    def processed_logits(self):
        """(B, V) rows the last pick read, or None while processors are off"""
        ptr = lib().gpt2_decode_processed_logits(self.h)
        if not ptr:
            return None
        out = np.empty((self.B, self.cfg.vocab_size), np.float32)
        check(lib().hpa_synchronize(), "synchronize")
        check(lib().hpa_memcpy(out.ctypes.data, ptr, out.nbytes), "processed logits download")
        return out

    def history(self, seq):
        """the tokens fed to sequence seq at positions [0, pos)"""
        n = ctypes.c_int()
        check(lib().gpt2_decode_history(self.h, int(seq), None, ctypes.byref(n)), "history")
        out = np.zeros(n.value, np.int32)
        if n.value:
            check(lib().gpt2_decode_history(self.h, int(seq), out.ctypes.data_as(_I), ctypes.byref(n)), "history")
        return out

    def token_counts(self, seq):
        """(V,) how often each token was fed to sequence seq inside its window"""
        out = np.zeros(self.cfg.vocab_size, np.int32)
        check(lib().gpt2_decode_token_counts(self.h, int(seq), out.ctypes.data_as(_I)), "token_counts")
        return out

    def gemm_config(self, waves=None, row_blocks=None, col_tiles=None):
        """fused GEMM launch shapes [qkv, attproj, fc, fcproj, logits]:
        (waves, 16-row blocks, 16-column tiles) per workgroup; applies the
        nonzero entries of the given lists first"""
        arrs = [np.ascontiguousarray(a if a is not None else [0] * 5, np.int32)
                for a in (waves, row_blocks, col_tiles)]
        if any(a is not None for a in (waves, row_blocks, col_tiles)):
            check(lib().gpt2_decode_gemm_config(self.h, *[a.ctypes.data_as(_I) for a in arrs], 1),
                  "gemm_config")
        out = [np.zeros(5, np.int32) for _ in range(3)]
        check(lib().gpt2_decode_gemm_config(self.h, *[a.ctypes.data_as(_I) for a in out], 0), "gemm_config")
        return tuple(out)

    def step_bytes(self):
        att = ctypes.c_double()
        tot = lib().gpt2_decode_step_bytes(self.h, ctypes.byref(att))
        return tot, att.value

    def reset(self):
        check(lib().gpt2_decode_reset(self.h), "reset")

    def reserve(self, ctx):
        check(lib().gpt2_decode_reserve(self.h, ctx), "reserve")

    def set_positions(self, pos):
        pos = np.ascontiguousarray(pos, np.int32)
        check(lib().gpt2_decode_set_positions(self.h, pos.ctypes.data_as(_I)), "set_positions")

    def fill_random(self, ctx, seed=1, seq_offset=0):
        """synthetic K/V of positions [0, ctx); seq_offset: this engine's rows
        are sequences seq_offset.. of a larger (sharded) batch"""
        check(lib().gpt2_decode_fill_random_ex(self.h, ctx, seed, seq_offset), "fill_random")

    def close(self):
        if self.h:
            lib().hpa_synchronize()
            lib().gpt2_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synthetic_params(cfg, seed=1337):
    L = lib()
    c = cfg if isinstance(cfg, GPT2Config) else config(cfg)
    n = L.gpt2_num_parameters(c)
    p = np.empty(n, np.float32)
    check(L.gpt2_synthetic_params(c, seed, p.ctypes.data_as(_F)), "synthetic_params")
    return p


class Timer:
    """HIP events on the library's stream (where the kernels run)."""

    def __init__(self):
        self.a = lib().hpa_event_create()
        self.b = lib().hpa_event_create()

    def start(self):
        check(lib().hpa_event_record(self.a), "event_record")

    def stop(self):
        check(lib().hpa_event_record(self.b), "event_record")
        return lib().hpa_event_elapsed_ms(self.a, self.b)

    def __del__(self):
        try:
            lib().hpa_event_destroy(self.a)
            lib().hpa_event_destroy(self.b)
        except Exception:
            pass
