// hpa_handoff.h -- the in-launch hand-off between workgroups of the persistent
// decode kernels (hpa_layer_units.hip, hpa_chain6.hip, hpa_chain8.hip,
// hpa_chain_b16.hip, hpa_pipe.hip), once.  Device code only.  (The bf16 chain
// and the pipelined halves use the constants, barriers and arrive of this
// header and keep a copy of the wait loop: see the note at their wait.)
//
// The protocol (MI355X_MICROARCH.md "Valid forms", row 1; cdna_hip_programming.md
// Guideline 16; DESIGN.md section 3 "Hand-off primitives"):
//   producer  every byte handed over is stored sc1 (write-through); each
//             storing wave drains (drain_vm), the workgroup meets at
//             lds_barrier, then ONE lane adds to the counter (arrive_shard, or
//             a kernel's own per-line add);
//   consumer  wave 0 polls the counter lines with agent-scope loads, the other
//             waves wait at a barrier (wait_wg); what was handed over is then
//             loaded sc1 (L1 bypass).
// Counters are zeroed before every step, one 128-B line per counter (shard).
// Every spin is bounded: after kSpinTicks the waiting workgroup writes its
// phase code to *err (and *err_sticky) and the launch ends, outputs garbage,
// reported by the host; the other workgroups see *err and follow.
#pragma once
#include "hpa_internal.h"

namespace hpa {

constexpr int kPad = 32;                    // ints per counter line / shard (one 128-B line)
constexpr long long kSpinTicks = 20000000;  // s_memrealtime is 100 MHz: 200 ms

// workgroup barrier that does not drain the vector-memory counter (weights
// prefetched across a seam stay in flight); LDS accesses before it are complete
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// every storing wave drained.  The builtin form, not inline asm: the
// compiler must know vmcnt is 0 here, or it waits again before the first
// register it reuses after the stores -- and vmcnt is in order, so that wait
// also drained the next phase's weight prefetch issued in between (seen in
// the gfx950 ISA of round 4: the prefetch had to land before the wait began)
__device__ __forceinline__ void drain_vm() {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) expcnt(7) lgkmcnt(15)
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// one lane, after every storing wave's drain and the workgroup barrier: add n
// to the workgroup's shard (of 8) of the counter at ctr
__device__ __forceinline__ void arrive_shard(int* ctr, int n) {
    __hip_atomic_fetch_add(ctr + (blockIdx.x & 7) * kPad, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// poll (wave 0): the 8 shards of the counter at ctr sum to `expected`.
// HPA_PL_POLL: experiment switches of A/B builds (results in DESIGN.md)
#ifndef HPA_PL_POLL
#define HPA_PL_POLL 0
#endif
__device__ __forceinline__ bool shards_reached(const int* c, int expected) {
    const int lane = threadIdx.x & 63;
#if HPA_PL_POLL == 2  /* experiment: returning atomic add of 0 (served at the memory side) */
    int v = lane < 8 ? __hip_atomic_fetch_add(const_cast<int*>(c) + lane * kPad, 0, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT)
                     : 0;
#elif HPA_PL_POLL == 3  /* experiment: system-scope (sc0 sc1) loads */
    int v = lane < 8 ? __hip_atomic_load(c + lane * kPad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0;
#else
    int v = lane < 8 ? __hip_atomic_load(c + lane * kPad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
#endif
    v = __builtin_amdgcn_readfirstlane(wave_sum_int(v));
    return v >= expected;
}

// The bounded spin, run by ONE wave: poll() (wave-uniform) until it is true.
// Every eighth poll reads the step's error word (another workgroup gave up:
// follow at once) and the clock; past kSpinTicks `code` goes to *err and
// *err_sticky.  false: gave up.  (err, err_sticky by reference: kernel
// arguments, read where used -- err_sticky only on the timeout path.)
template <typename Poll>
__device__ __forceinline__ bool spin_bounded(int* const& err, int* const& err_sticky, int code, Poll&& poll) {
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    for (unsigned it = 0;; ++it) {
        if (poll()) return true;
        if ((it & 7) == 7) {
            const int e = __builtin_amdgcn_readfirstlane(__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (e) return false;  // another workgroup gave up: follow at once
            if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > kSpinTicks) {
                if ((threadIdx.x & 63) == 0) {
                    atomicCAS(err, 0, code);
                    if (err_sticky) atomicCAS(err_sticky, 0, code);
                }
                return false;
            }
        }
#ifndef HPA_PL_NOSLEEP  // experiment switch of A/B builds
        __builtin_amdgcn_s_sleep(1);
#endif
    }
}

// every thread of the workgroup calls; wave 0 spins on poll (evaluated by
// wave 0 only), the rest wait at the barrier; s_ok is a word of LDS
template <typename Poll>
__device__ __forceinline__ bool wait_wg(int* const& err, int* const& err_sticky, int code, int& s_ok, Poll&& poll) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wv == 0) {
        const int ok = spin_bounded(err, err_sticky, code, poll) ? 1 : 0;
        if ((threadIdx.x & 63) == 0) s_ok = ok;
    }
    lds_barrier();
    const bool ok = s_ok != 0;
    lds_barrier();  // s_ok read before the next wait rewrites it
    return ok;
}

}  // namespace hpa
