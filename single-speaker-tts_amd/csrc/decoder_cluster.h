// What the two persistent decoders (decoder_persistent.hip, decoder_ws.hip) share: the cluster hand-off, the layout of its
// sync words, and the window of LocalLuongAttention (which decoder.hip uses as well).
//
// The hand-off.  Activations travel between the workgroups of a cluster through small global buffers with the write-through
// hand-off of MI355X_MICROARCH.md ("valid forms"):
//   * every handed-off byte is stored sc1 (dc_st4);
//   * every storing wave waits vmcnt(0) and adds to the cluster's counter (agent scope) for itself (dc_publish_wave); a phase
//     whose waves all store keeps drain -> barrier -> one add (dc_publish).  A workgroup counts DC_ARRIVALS per phase either way;
//   * consumers poll that counter with an sc1 load in one lane, then a workgroup barrier (dc_wait), then sc1 loads of the
//     bytes (dc_ld4).  No cache-wide release or acquire anywhere, no grid-wide barrier: clusters never talk to each other;
//   * every wait is bounded (DC_SPIN_LIMIT polls); on a timeout the status word is set, every workgroup of the grid sees it at
//     its next wait and the kernel drains.  The word is sticky: no launch clears it, the host does when it has read it.
// All workgroups must be co-resident; each counts itself on the resident word when it starts (dc_all_resident).
#pragma once
#include <cstddef>
#ifdef __HIPCC__
#include "tts_common.h"
#include "decoder.h"
#endif

namespace tts {

// ---- sync words of a launch (plain C++): one arrival counter per cluster, DC_CNT_LD words apart (a counter has its cache lines to
// itself), then the resident count, then the sticky status word.  Counters and resident count are zeroed per launch.
#define DC_CNT_LD 64
inline size_t dc_resident_index(int clusters) { return (size_t)DC_CNT_LD * clusters; }
inline size_t dc_status_index(int clusters) { return dc_resident_index(clusters) + 1; }
inline size_t dc_sync_words(int clusters) { return dc_status_index(clusters) + 1; }
inline size_t dc_zeroed_words(int clusters) { return dc_status_index(clusters); }   // everything in front of the status word
// The weight-stationary launch lays its words out for sync_clusters >= its own cluster count: one place for the status word
// of both of its forms at one batch size, so that a status raised by a launch of one is found after a launch of the other.
inline int dc_layout_clusters(int clusters, int sync_clusters) { return sync_clusters < clusters ? clusters : sync_clusters; }
struct DcSync { unsigned* counters; unsigned* resident; int* status; };
inline DcSync dc_sync(unsigned* sync, int clusters) {
    return {sync, sync + dc_resident_index(clusters), reinterpret_cast<int*>(sync + dc_status_index(clusters))};
}

// ---- the window of LocalLuongAttention (reference attention.py:32-342): 2D+1 positions [w_lo, w_lo + w_n).  (constexpr: host
// and device)
// MONOTONIC mode at decoder step t (attention.py:263-286): p = min(max(t, D), Ts - (D + 1)), window [p - D, p + D + 1).
// Needs Ts >= 2D + 1 (checked by the callers).
constexpr int local_center(int t, int Ts, int D) {
    int p = t > D ? t : D;
    const int hi = Ts - (D + 1);
    return p < hi ? p : hi;
}
// PREDICTIVE mode (attention.py:246-258), c = floor(p): a window that leaves the memory is where the reference stops being
// well defined (its padding arithmetic, attention.py:288-304, fails at run time) -- the callers raise the error flag and
// score the window clamped into the memory.
constexpr bool local_inside_memory(int c, int D, int Ts) { return c - D >= 0 && c + D + 1 <= Ts; }
constexpr int local_clamped_lo(int c, int D, int Ts, int w_n) {
    const int lo = c - D > 0 ? c - D : 0;
    return lo < Ts - w_n ? lo : Ts - w_n;
}

#ifdef __HIPCC__
// The per-step arguments of the local form
struct DcLocal {
    int d, gaussian, predictive, step;
    const float* wp; const float* vp;   // [256][256] (q @ W_p), [256]
    float* p_hist_t;                    // [B] predicted centres of this step
    int* err_flag;
};

// luong_force_gaussian: the reported alignments (not the context) are weighted by exp(-(j - p)^2 / 2 * (D/2)^2), the
// reference's expression as written (attention.py:73-80)
__device__ __forceinline__ float local_gauss_k(int D) { return 0.5f * (0.5f * D) * (0.5f * D); }
__device__ __forceinline__ float local_gauss(float j, float p, float gk) {
    const float dist = j - p;
    return __expf(-(dist * dist) * gk);
}

// Predicted centre, a row's partial sum: (q W_p)[n] by thread n of the row's 256, then this wave's part of v_p . tanh(.), in
// double (tts_common.h, predicted_centre).  Two accumulators: dec_predict_centre_kernel sums in another order.
__device__ __forceinline__ double local_predict_wave_sum(const float* qs, const float* wp, const float* vp, int n) {
    constexpr int A = 256;
    double a0 = 0.0, a1 = 0.0;
    const float* wpn = wp + n;
    for (int k = 0; k < A; k += 2) {
        a0 = fma((double)qs[k], (double)wpn[(size_t)k * A], a0);
        a1 = fma((double)qs[k + 1], (double)wpn[(size_t)(k + 1) * A], a1);
    }
    return wave_sum_f64((double)tanhf((float)(a0 + a1)) * (double)vp[n]);
}

// ---- device side of the hand-off
#define DC_SPIN_LIMIT 2000000u   // polls of ~1 us each
#define DC_ARRIVALS 2u           // what a workgroup adds to its cluster's counter per phase, however many of its waves store
typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned dc_u32x4;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t dc_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)0xFFFFFFF0u, 0x00020000);
}
// 16-byte sc1 (write-through / L1-bypassing) accesses: aux bit 4
__device__ __forceinline__ float4 dc_ld4(const __amdgpu_buffer_rsrc_t& rs, unsigned byte_off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, 16));
}
__device__ __forceinline__ void dc_st4(const __amdgpu_buffer_rsrc_t& rs, unsigned byte_off, float4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(dc_u32x4, v), rs, (int)byte_off, 0, 16);
}

// Thread 0 of a workgroup, once: this workgroup has started -- was it the last of the grid?  With all of them resident the
// CUs the call pipeline held for this stream are no longer needed: the kernel raises its hold flag (reserve.hip) with
//     if (dc_all_resident(p.resident) && p.hold_flag) dc_release_held(p.hold_flag);
__device__ __forceinline__ bool dc_all_resident(unsigned* resident) {
    const unsigned n = __hip_atomic_fetch_add(resident, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return n + 1 == gridDim.x;
}
__device__ __forceinline__ void dc_release_held(int* hold_flag) { __hip_atomic_store(hold_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Start of a phase: wait until `target` arrivals have been counted on the cluster's counter (lane 0 polls, everybody
// meets at the barrier).  The arrival of THIS workgroup for the previous phase was signalled when that phase ended:
// until round 4 it was signalled here, behind the next phase's weight requests and address arithmetic -- 1.0-1.4 us in
// which the peers could not yet see that this workgroup was done, on every phase's critical path.
// ctrl: one LDS word of the workgroup, zero at the start.
__device__ __forceinline__ void dc_wait(unsigned* cnt, unsigned target, int* status, int* ctrl) {
    if (threadIdx.x == 0 && target > 0) {
        if (ctrl[0] == 0) {
            unsigned spins = 0;
            while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                __builtin_amdgcn_s_sleep(1);
                if ((++spins & 1023u) == 0 &&
                    (spins > DC_SPIN_LIMIT || __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                    __hip_atomic_store(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ctrl[0] = 1;   // drain: no further waits in this workgroup
                    break;
                }
            }
        }
    }
    __syncthreads();
}

// End of a phase in which every wave stores: each waits for its (write-through) stores, then the workgroup barrier -- after
// it one lane signals for all of them: the arrival on the cluster's counter (agent scope), at once.
__device__ __forceinline__ void dc_publish(unsigned* cnt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(cnt, DC_ARRIVALS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The same for a phase whose stores all come from a few of its waves (the GEMM phases' epilogue): every storing wave signals
// its share of DC_ARRIVALS for itself when ITS stores have drained (MI355X_MICROARCH.md, valid forms: "each storing wave
// for itself"), and no workgroup barrier stands between the other waves and the next phase's weight requests: those are in
// flight while the epilogue runs, not behind it (round 4: 14.9 -> 13.6 ms alone).  (What the barrier also did -- keep the
// partial tiles and the staged tile from being overwritten under the epilogue's reads -- the next phase's own barrier does:
// nobody writes either before dc_wait, and a phase that continues on the staged tile is entered through a barrier.)
__device__ __forceinline__ void dc_publish_wave(unsigned* cnt, unsigned arrivals) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(cnt, arrivals, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- host side of a launch: what both enqueue functions write into their kernel's parameters (PdParams / WsParams) and clear
// on the stream.  The sync words: counters and resident count start at zero for every launch; the status word behind them is
// sticky (the host clears it when it has read it, api_handle.hip), so a timeout is not lost when several calls are queued before
// a sync.  LocalLuongAttention: the predictive mode needs both buffers, and its error flag starts at zero for every launch.
template <class Params>
inline hipError_t dc_launch_params(hipStream_t s, unsigned* sync, int clusters, const DecoderWeights& w, float* p_hist, int* err_flag,
                                   Params& p) {
    const DcSync v = dc_sync(sync, clusters);
    p.counters = v.counters; p.resident = v.resident; p.status = v.status;
    p.local_d = w.local_d; p.local_gaussian = w.local_gaussian; p.local_predictive = w.local_d > 0 && w.local_predictive;
    p.local_wp = w.local_wp; p.local_vp = w.local_vp; p.p_hist = p_hist; p.err_flag = err_flag;
    if (p.local_predictive && (!p_hist || !err_flag)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(sync, 0, dc_zeroed_words(clusters) * sizeof(unsigned), s);
    if (e == hipSuccess && p.local_predictive) e = hipMemsetAsync(err_flag, 0, sizeof(int), s);
    return e;
}
#endif   // __HIPCC__

}  // namespace tts
