// hpa_park.hip -- whole pages between the pool and one contiguous buffer
// (hpa_pool_gather_pages / hpa_pool_scatter_pages): the data path of
// gpt2_decode_park / gpt2_decode_unpark.
#include "hpa_internal.h"

// Page i of layer l of the buffer sits at byte (l * n_pages + i) * page_bytes,
// wherever the page sat in the pool.  Grid (16-byte chunks, layer, page of this
// launch), the launch's page ids by value in the kernel arguments, as
// pool_copy_pages_kernel: lane i of a wave moves chunk base + i, so one store
// instruction writes 1 KiB of consecutive bytes (whole lines of host memory
// when the buffer is pinned), 4 chunks per thread, every load issued before
// the first store.  Every address is size_t arithmetic from the first product
// on (pools past 2^31 / 2^32 / 2^33 bytes a layer).
struct ParkPages {
    int slot[HPA_PARK_MAX_PAGES];
};
constexpr int kParkThreads = 256, kParkUnroll = 4;
typedef unsigned park_u32x4 __attribute__((ext_vector_type(4)));

// NT: the pool side of the move is non-temporal (the gather's loads, the
// scatter's stores); hpa_park_set_nontemporal picks it at run time
template <bool SCATTER, bool NT>
__global__ __launch_bounds__(kParkThreads) void park_pages_kernel(char* __restrict__ pool_base, size_t layer_bytes,
                                                                  size_t page_bytes, unsigned chunks,
                                                                  char* __restrict__ buf, unsigned first,
                                                                  unsigned n_pages, const ParkPages pages) {
    const size_t pool_off = (size_t)blockIdx.y * layer_bytes + (size_t)pages.slot[blockIdx.z] * page_bytes;
    const size_t buf_off = ((size_t)blockIdx.y * (size_t)n_pages + (size_t)first + (size_t)blockIdx.z) * page_bytes;
    park_u32x4* __restrict__ p = reinterpret_cast<park_u32x4*>(pool_base + pool_off);
    park_u32x4* __restrict__ b = reinterpret_cast<park_u32x4*>(buf + buf_off);
    const unsigned i0 = blockIdx.x * (kParkThreads * kParkUnroll) + threadIdx.x;
    park_u32x4 v[kParkUnroll];
#pragma unroll
    for (int u = 0; u < kParkUnroll; ++u) {
        const unsigned i = i0 + u * kParkThreads;
        if (i < chunks) {
            if (SCATTER) v[u] = b[i];
            else if (NT) v[u] = __builtin_nontemporal_load(p + i);
            else v[u] = p[i];
        }
    }
#pragma unroll
    for (int u = 0; u < kParkUnroll; ++u) {
        const unsigned i = i0 + u * kParkThreads;
        if (i < chunks) {
            if (!SCATTER) b[i] = v[u];
            else if (NT) __builtin_nontemporal_store(v[u], p + i);
            else p[i] = v[u];
        }
    }
}

// bit 0: the gather's loads, bit 1: the scatter's stores.  Measured (profiles/r18/park.txt, two runs, the
// second recorded; profiles/EXPERIMENTS.md has both): non-temporal loads make the gather 1.7-6 % faster at all
// six shapes in both runs; non-temporal stores make the scatter 1.4-4.5 % faster at n = 100 in both runs and at
// n = 1000 0.6-3 % faster in one run, 1.9-5 % slower in the other (box to box), so for the scatter it is a wash
static int g_park_nt = 3;

static int park_launch(const HpaKVPool* pool, const int* pages, int n_pages, void* buf, bool scatter) {
    HPA_REQUIRE(pool && pool->base && pages && buf, "park: pool, page list, buffer");
    HPA_REQUIRE(n_pages >= 1, "park: n_pages >= 1");
    const size_t page_bytes = pool->page_elems * pool->elem_bytes;
    HPA_REQUIRE(page_bytes % 16 == 0 && page_bytes / 16 <= 0xffffffffu, "park: page bytes");
    HPA_REQUIRE((size_t)buf % 16 == 0, "park: the buffer must be 16-byte aligned");
    HPA_REQUIRE(pool->num_layers >= 1 && pool->num_layers <= 65535, "park: too many layers");
    for (int i = 0; i < n_pages; ++i)
        HPA_REQUIRE(pages[i] >= 0 && pages[i] < pool->num_pages, "park: page out of range");
    if (scatter)  // a slot written twice would hold whichever store lands last (a page list is short: in place)
        for (int i = 1; i < n_pages; ++i)
            for (int j = 0; j < i; ++j) HPA_REQUIRE(pages[i] != pages[j], "scatter_pages: a page appears twice");
    HPA_REQUIRE(hpa_is_device_accessible(buf), "park: the buffer is not device-accessible (device or pinned host)");
    // the last byte too: a registered range may end inside the buffer
    HPA_REQUIRE(hpa_is_device_accessible((const char*)buf + hpa_park_bytes(pool, n_pages) - 1),
                "park: the buffer's end is not device-accessible");
    const unsigned chunks = (unsigned)(page_bytes / 16);
    const unsigned per_block = kParkThreads * kParkUnroll;
    const size_t layer_bytes = pool->layer_elems * pool->elem_bytes;
    const bool nt = scatter ? (g_park_nt & 2) != 0 : (g_park_nt & 1) != 0;
    for (int first = 0; first < n_pages; first += HPA_PARK_MAX_PAGES) {
        const int n = n_pages - first < HPA_PARK_MAX_PAGES ? n_pages - first : HPA_PARK_MAX_PAGES;
        ParkPages pp;
        for (int i = 0; i < HPA_PARK_MAX_PAGES; ++i) pp.slot[i] = i < n ? pages[first + i] : 0;  // past n never read: grid.z = n
        const dim3 grid((chunks + per_block - 1) / per_block, (unsigned)pool->num_layers, (unsigned)n);
#define PARK_LAUNCH(S, N)                                                                                             \
    park_pages_kernel<S, N><<<grid, kParkThreads, 0, hpa_stream()>>>((char*)pool->base, layer_bytes, page_bytes,     \
                                                                     chunks, (char*)buf, (unsigned)first,            \
                                                                     (unsigned)n_pages, pp)
        if (scatter) {
            if (nt) PARK_LAUNCH(true, true);
            else PARK_LAUNCH(true, false);
        } else {
            if (nt) PARK_LAUNCH(false, true);
            else PARK_LAUNCH(false, false);
        }
#undef PARK_LAUNCH
        HPA_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" {

size_t hpa_park_bytes(const HpaKVPool* pool, int n_pages) {
    if (!pool || n_pages < 0) return 0;
    return (size_t)pool->num_layers * (size_t)n_pages * (pool->page_elems * pool->elem_bytes);
}

size_t hpa_park_offset(const HpaKVPool* pool, int n_pages, int layer, int i) {
    if (!pool) return 0;
    return ((size_t)layer * (size_t)n_pages + (size_t)i) * (pool->page_elems * pool->elem_bytes);
}

int hpa_pool_gather_pages(const HpaKVPool* pool, const int* pages, int n_pages, void* dst) {
    return park_launch(pool, pages, n_pages, dst, false);
}

int hpa_pool_scatter_pages(const HpaKVPool* pool, const int* pages, int n_pages, const void* src) {
    return park_launch(pool, pages, n_pages, const_cast<void*>(src), true);
}

int hpa_park_set_nontemporal(int mask) {
    HPA_REQUIRE(mask >= 0 && mask <= 3, "park_set_nontemporal: mask 0..3");
    g_park_nt = mask;
    return 0;
}

int hpa_park_nontemporal(void) { return g_park_nt; }

}  // extern "C"
