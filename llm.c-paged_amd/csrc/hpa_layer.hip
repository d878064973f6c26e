// hpa_layer.hip -- hpa_decode_layer, the decode step's layer as one
// persistent launch (gfx950): the extern "C" surface.  The forms live in
// hpa_layer_units.hip (0..5: units of 4, 6 or 12 waves, with or without the
// attention), hpa_chain6.hip (6: the default at C = 768, and the step's first
// launch) and hpa_chain8.hip (8: wide layers); what they share is in
// hpa_layer_common.h, the hand-off protocol in hpa_handoff.h (DESIGN.md
// section 3).
#include "hpa_layer_common.h"

namespace {
template <int NH>
bool shape_ok(int B, int S, int G) {
    // one unit per slot in every phase: attention B*NH*S, fc and fcproj
    // 4*(C/16)*R units; grid and unit numbering assume G % 8 == 0
    const int R = (B + 15) / 16;
    return B >= 1 && B <= 64 && S >= 1 && S <= HPA_ATTN_MAX_SPLITS && G % 8 == 0 && (long)B * NH * S <= 3L * G &&
           4L * LD<NH>::NCT * R <= 3L * G;
}

}  // namespace

#ifdef HPA_LAYER_TRACE
int hpa_pl_trace_add(const void* sym, unsigned long long* host, int layers) {
    static unsigned long long buf[64 * 256 * 16];
    const size_t n = (size_t)layers * 256 * 16;
    if (!host) {
        memset(buf, 0, sizeof(buf));
        HPA_CHECK(hipMemcpyToSymbol(sym, buf, sizeof(buf)));
        return 0;
    }
    HPA_CHECK(hipMemcpyFromSymbol(buf, sym, n * 8));
    for (size_t i = 0; i < n; ++i) host[i] += buf[i];
    return 0;
}
#endif

extern "C" {

int hpa_decode_layer_eligible_cus(int B, int C, int num_heads, int splits, int G) {
    if (G <= 0 || C != 64 * num_heads) return 0;
    if (num_heads == 12) return shape_ok<12>(B, splits, G) ? 1 : 0;
    if (num_heads == 2) return shape_ok<2>(B, splits, G) ? 1 : 0;
    return 0;
}
int hpa_decode_layer_eligible(int B, int C, int num_heads, int splits) {
    return hpa_decode_layer_eligible_cus(B, C, num_heads, splits, hpa::num_cus());
}

// the split count measured best for the stand-alone attention
// (hpa_attn_pick_splits: a range of >= 4 tiles per 4-wave unit; short ranges
// pay the merge), halved until every unit has a slot (B*NH*S <= 3 x CUs)
int hpa_decode_layer_pick_splits_cus(int B, int num_heads, int max_ctx, int G) {
    if (G <= 0 || B <= 0 || num_heads <= 0) return 1;
    int s = hpa_attn_pick_splits(B, num_heads, max_ctx, G);
    while (s > 1 && (long)B * num_heads * s > 3L * G) s /= 2;
    return s;
}
int hpa_decode_layer_pick_splits(int B, int num_heads, int max_ctx) {
    return hpa_decode_layer_pick_splits_cus(B, num_heads, max_ctx, hpa::num_cus());
}

int hpa_decode_layer_sizes(int B, int C, int num_heads, int splits, size_t* out3) {
    HPA_REQUIRE(out3 && B > 0 && C == 64 * num_heads && splits >= 1, "decode layer sizes: bad arguments");
    const int R = (B + 15) / 16, nct = C / 16;
    out3[0] = (size_t)B * num_heads * splits * kRec;
    out3[1] = (size_t)4 * R * nct * 256;  // fcproj K-part partial tiles
    const size_t ints5 = (size_t)kCtrInts + 2 * (size_t)R * nct + (size_t)B * num_heads;
    const size_t ints6 = (size_t)chain::kCtr + (size_t)4 * nct + chain::kGrp;  // form 6: counters, tickets [4][nct], k-groups
    const size_t ints = ints5 > ints6 ? ints5 : ints6;
    out3[2] = (ints + 31) / 32 * 32;  // whole 128-B lines (memset in multiples of 16 B)
    return 0;
}

// trace build only: copy the per-(layer, workgroup) event stamps of the last
// launches ([layers][256][16] u64, s_memrealtime ticks of 10 ns); host NULL
// clears them.  Returns 1 in the product build.
int hpa_decode_layer_trace(unsigned long long* host, int layers) {
#ifdef HPA_LAYER_TRACE
    HPA_REQUIRE(layers >= 0 && layers <= 64, "trace: layers 0..64");
    // each kernel file has its own stamps; one form runs in a traced step, so their sum is that form's
    if (host) memset(host, 0, (size_t)layers * 256 * 16 * 8);
    return hpa_layer_units_trace(host, layers) || hpa_chain6_trace(host, layers) || hpa_chain8_trace(host, layers);
#else
    (void)host;
    (void)layers;
    return 1;
#endif
}

// the chain forms 6 (C = 768) and 8 (C = 768, 1024, 1280 or 1600): B <= 64, fp32 or
// bf16 pool (form 6: fp8 too), a unit per workgroup in every phase
int hpa_decode_chain_eligible_cus(int B, int C, int num_heads, int form, int G) {
    if (G <= 0 || C != 64 * num_heads || B < 1 || B > 64) return 0;
    if (form == 6) {
        if (num_heads != 12) return 0;
        const int R = (B + 15) / 16;
        return R * 48 <= G && 4 * R * 48 / (R == 1 ? 1 : R == 2 ? 2 : 3) <= G ? 1 : 0;
    }
    if (form == 8) {  // GPT-2 124M / medium / large / XL widths (C = 768, 1024, 1280, 1600)
        if (num_heads != 12 && num_heads != 16 && num_heads != 20 && num_heads != 25) return 0;
        int xt[4], xng[4];
        return hpa_chain8_shape(B, num_heads, G, xt, xng) == 0 ? 1 : 0;
    }
    return 0;
}
int hpa_decode_chain_eligible(int B, int C, int num_heads, int form) {
    return hpa_decode_chain_eligible_cus(B, C, num_heads, form, hpa::num_cus());
}

int hpa_decode_layer(const HpaLayerArgs* h) {
    HPA_REQUIRE(h && h->pool && h->pool->base, "decode layer: pool");
    const HpaKVPool* pool = h->pool;
    // fp8 pools: chain form 6 only (its qkv epilogue stores the codes); the other forms are fp32 / bf16
    HPA_REQUIRE(pool->dtype == HPA_F32 || pool->dtype == HPA_BF16 ||
                    (pool->dtype == HPA_FP8 && h->chain_only == 6 && pool->scales && pool->page_size % 16 == 0),
                "decode layer: fp32 or bf16 pool (fp8: chain form 6, pages of 16, 32, 64)");
    HPA_REQUIRE(pool->head_size == HS && h->C == h->num_heads * HS, "decode layer: head size 64");
    HPA_REQUIRE(h->layer >= 0 && h->layer < pool->num_layers && (h->last || h->layer + 1 < pool->num_layers),
                "decode layer: layer out of range");
    HPA_REQUIRE(h->q && h->att && h->res && h->res2 && h->fch && h->w_ap && h->b_ap && h->w_fc && h->fc_c1 &&
                    h->fc_c2 && h->w_fp && h->b_fp && h->block_table && h->pos && h->rec && h->slab &&
                    h->counters && h->err,
                "decode layer: null operand");
    HPA_REQUIRE(h->last || (h->w_qkv && h->qkv_c1 && h->qkv_c2 && h->q_out), "decode layer: qkv(l+1) operands");
    HPA_REQUIRE(h->splits >= 1 && h->splits <= HPA_ATTN_MAX_SPLITS, "decode layer: splits 1..16");
    const int G = hpa::num_cus();
    if (h->chain_only == 6 || h->chain_only == 8) {
        HPA_REQUIRE(hpa_decode_chain_eligible(h->B, h->C, h->num_heads, h->chain_only),
                    "decode layer: chain form not supported for this shape");
        return h->chain_only == 8 ? hpa_chain8_launch(h, G) : hpa_chain6_launch(h, G);
    }
    HPA_REQUIRE(hpa_decode_layer_eligible(h->B, h->C, h->num_heads, h->splits), "decode layer: shape not supported");
    return hpa_layer_units_launch(h, G);
}

}  // extern "C"
