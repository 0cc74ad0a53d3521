// Griffin-Lim phase reconstruction, STFT analysis and the spectrogram de-normalisation (gfx950).
//
// Replaces, batched and on device:
//   griffin_lim_v2 / spectrogram_to_wav   reference audio/synthesis.py:43-125, 5-40
//     (librosa.istft + librosa.stft per iteration, a per-frame Python loop in the reference)
//   inv_normalize_decibel / decibel_to_magnitude / ** power
//                                          reference audio/conversion.py:81-102, 32-53,
//                                          tacotron/inference.py:93-101, 175
//   librosa.output.write_wav(norm=True)    reference audio/io.py:53 (peak normalisation)
//   linear_scale_spectrogram / mel         reference audio/features.py:5-86, 116-145
//
// Internal layout: frame-major.  mag [B][T][FP] float and a ping-pong pair of 32-bit unit-phasor codes
// e^{i phi} [B][T][FP] (gl_pack_phasor; the estimate X = |S| e^{i phi} is rebuilt from mag where it is
// consumed), FP = 1056 (F = 1025 padded so that every row starts on a 128-byte line: -2.5 % per launch).  One frame's spectrum is a
// contiguous row, which is also how the network produces it (B,T,F): the reference's (F,T) transpose
// exists only at the C ABI.
//
// One launch runs one to three Griffin-Lim iterations on PERSISTENT workgroups (512 threads, one per compute unit) that
// draw RUNS of consecutive frames of one utterance from a global counter: gl_stream_kernel, described where it is
// defined.  The time-domain signal never goes to HBM; per bin and iteration the ALGORITHMIC traffic (what the
// roofline is priced on) is 8 B X in + 4 B |S| + 8 B X out; what really moves with three iterations per launch is a
// 4-byte phasor code in and out per launch plus |S|.  The cut of an utterance into runs is planned on the host:
// gl_plan_items (gl_plan.hip).
//
// FFT: real 2048-point transforms as 1024-point complex FFTs with a split/merge pass.  One wave
// per FFT, 16 points per lane: radix-16 in registers -> 4x4 register/lane transpose (v_permlane16_swap /
// v_permlane32_swap) -> radix-4 -> LDS transpose -> radix-16; all twiddles and this lane's window samples
// (with the iFFT scale folded in) in registers.  Index math validated against numpy in
// tests/test_host_logic.py (test_fft_decomposition_emulation).  Complex numbers are packed values (v_pk_add /
// v_pk_mul / v_pk_fma_f32 with op_sel / neg modifiers, see "complex helpers"): the kernel is bound by VALU issue
// (one instruction per ~4 cycles and SIMD whatever it is), and a packed instruction costs about as much as a
// scalar one.  This file is still compiled with -fno-slp-vectorize: what the SLP vectoriser packs on its own
// (unrelated scalars, with v_mov shuffles to align the pairs) is slower than leaving it scalar.
#include "tts_common.h"
#include "griffin_lim.h"
#include "fft_wave.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace tts {

// complex helpers, butterflies, fft16 / fft1024: fft_wave.h

// Workgroup barrier that orders LDS accesses only.  __syncthreads() also waits for every outstanding global
// load and STORE of the wave (s_waitcnt vmcnt(0)); at the end of phase B that is the full HBM write latency of a
// frame's spectrum row, three times per chunk, for nothing: no wave ever reads what another wave stored to
// global memory inside this kernel.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Progress flags of the overlap-add (LDS words polled / written by single lanes).  The pointer is cast to the LDS
// address space explicitly: a `volatile int*` derived from the dynamic shared array stays a GENERIC pointer (address
// space inference skips volatile accesses), and the access becomes flat_load / flat_store ... sc0 sc1 followed by
// s_waitcnt vmcnt(0) -- every round then waits for the next frame's prefetched spectrum row before its overlap-add
// instead of in the next round's unpacking.  These are ds_read_b32 / ds_write_b32 and touch lgkmcnt only.
typedef __attribute__((address_space(3))) int gl_lds_int;
__device__ __forceinline__ int gl_flag_load(int* p) {
    return __hip_atomic_load((gl_lds_int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void gl_flag_store(int* p, int v) {
    __hip_atomic_store((gl_lds_int*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Bins MH - k of a spectrum row whose bins k = lane + 64 c this lane holds in z[c]: m[c] = Z[MH - lane - 64 c],
// through the wave's exchange buffer (one pass of 8-byte writes and reads).  Bin MH itself (wanted by lane 0,
// c = 0) is in no register: the caller passes it.
__device__ __forceinline__ void mirror_bins(const cf (&z)[16], cf (&m)[16], cf* ex, int lane, cf nyq) {
    cf* wr = ex + lane;
    const cf* rd = ex + (1024 - lane);
#pragma unroll
    for (int c = 0; c < 16; ++c) wr[64 * c] = z[c];
    if (lane == 0) ex[1024] = nyq;
    wave_lds_sync();
#pragma unroll
    for (int c = 0; c < 16; ++c) m[c] = rd[-64 * c];
    wave_lds_sync();
}

// ------------------------------------------------------------------------------------ GL iteration
// PAIR-OWNER layout of a spectrum row inside the streaming kernel (round 4).  The real-FFT merge and split passes couple bin
// k with bin MH - k: X[k] and X[MH - k] come from the same (Z[k], Z[MH - k]) with ONE twiddle product,
//     E = Z[k] + conj Z[MH-k],  o = W^k (Z[k] - conj Z[MH-k]):   2 X[k] = E - i o,   2 X[MH-k] = conj(E + i o)
// and likewise the two inputs of the inverse transform from (G[k], G[MH-k]).  So a lane OWNS the eight pairs of its bins
// k = lane + 64 c, c < 8 (k < 512): slot c of a row register set holds bin k, slot 8 + c bin MH - k (for lane 0, c = 0 that
// is the Nyquist bin MH; bin 512, its own mirror, is lane 0's extra `mid` value).  Magnitudes and phasor codes are loaded
// and stored straight in this layout (the mirrored half is a descending, still contiguous 256-byte access), the
// normalisation works on it unchanged, and only half of a transform's values cross lanes: the forward FFT's upper
// registers (bins >= 512) go to their owners, the owners send the inverse FFT's upper inputs back.  6 VALU instructions per
// PAIR and 8 + 8 LDS accesses per pass instead of 5 per BIN and 16 + 16 (every lane fetching the mirror of each of its 16
// bins and multiplying by its twiddle): -64 VALU and -32 LDS instructions per frame and iteration.
#define GL_BIN(lane, j) ((j) < 8 ? (lane) + 64 * (j) : MH - (lane) - 64 * ((j) - 8))
// element j of a row through its two lane bases LO = row + lane, HI = row + (MH - lane): the offsets are instruction constants
#define GL_ROW(LO, HI, j) ((j) < 8 ? (LO)[64 * (j)] : (HI)[-64 * ((j) - 8)])
#define GL_THREADS 512     // GL_NW waves; NFFT, MH, GL_NW: gl_plan.h

// The spectra are streamed once per iteration (1.3 GB per launch at the bench size): non-temporal accesses
// keep them from evicting the decoder's weights and attention memory, which the second stream re-reads
// every step while this kernel runs.
__device__ __forceinline__ float gl_stream_load(const float* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void gl_stream_store(cf* p, cf v) { __builtin_nontemporal_store(v, p); }
#define GL_STREAM_LOAD(ptr) gl_stream_load(ptr)
#define GL_STREAM_STORE(ptr, val) gl_stream_store((ptr), (val))
// The state between iterations is the UNIT PHASOR of every bin, 32 bits each (round 2; the estimate X = |S| e^{i phi} it
// stands for is rebuilt in phase A from |S|, which phase A reads anyway from then on and phase B no longer does:
// 4 B phasor + 4 B |S| in, 4 B phasor out = 12 instead of 20 bytes per bin and iteration through a memory path that
// gives a compute unit ~21 GB/s however many waves ask, tools/stream_microbench.hip).  Code (round 4, second form): the
// point where the phasor's ray meets the diamond |Re| + |Im| = 1, stored as its imaginary part p = Im / (|Re| + |Im|)
// (|p| <= 1, a float) whose lowest mantissa bit carries the sign of Re.  Decoding: |Re| = 1 - |p| on the diamond, then
// one reciprocal square root of p^2 + (1 - |p|)^2 (between 1/2 and 1: well conditioned everywhere) brings the point
// back to the circle, times |S|.  No normalisation by |x| is needed to encode (the ratio does not see the scale), no
// compare and no select at either end, and the zero bin needs no special path: 0 / max(0, tiny) = 0 decodes to (1, 0),
// numpy's exp(1j * angle(0)) (and -0.0 + 0j to (-1, 0), also numpy's).  6 + 7 VALU instructions per bin and launch (the
// first form -- the smaller component over the larger, two flag bits -- took 11 + 10).  Worst-case error of a decoded
// component 4e-7 (one dropped mantissa bit of p, one v_rcp_f32, one v_rsq_f32; tests/test_host_logic.py::
// test_phasor_code_emulation), the size of the rounding in the x * rsq(|x|^2) * |S| product it replaces.
// Seeded start: the initial phasor e^{2 pi i u} of a bin, u = 24 bits of a 32-bit mix (lowbias32) of the seed and the
// bin's index in the reference's (B, F, T) layout.  The reference draws np.random.rand per call (audio/synthesis.py:91);
// a counter-based draw gives every bin its number wherever it is needed, so the first Griffin-Lim launch of a call makes
// its own initial estimate instead of reading 4 bytes per bin that another kernel wrote.  v_sin_f32 / v_cos_f32 take
// revolutions; their ~1e-6 error is a perturbation of a random angle.
__device__ __forceinline__ cf gl_seed_phasor(unsigned long long seed, unsigned long long idx) {
    unsigned x = (unsigned)idx ^ ((unsigned)(idx >> 32) * 0x9E3779B9u) ^ (unsigned)seed ^ ((unsigned)(seed >> 32) * 0x85EBCA6Bu);
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    const float u = (float)(x >> 8) * (1.0f / 16777216.0f);
    return cmk(__builtin_amdgcn_cosf(u), __builtin_amdgcn_sinf(u));
}
__device__ __forceinline__ unsigned gl_pack_phasor(cf x) {   // x: any scale
    // p = Im / (|Re| + |Im|), bit 0 = sign of Re (6 VALU instructions; see the comment above gl_seed_phasor)
    const float den = fmaxf(fabsf(x.x) + fabsf(x.y), 1.0e-30f);
    const float p = x.y * __builtin_amdgcn_rcpf(den);
    return (__float_as_uint(p) & ~1u) | (__float_as_uint(x.x) >> 31);
}
// mag >= 0 (every producer of the internal magnitude buffer writes |S|: gl_to_internal_kernel, the de-normalising
// epilogues).  The flag bit is NOT stripped from p before it is used: one ulp of p, exactly what stripping (a
// truncation) costs.  7 VALU instructions.
__device__ __forceinline__ cf gl_unpack_phasor(unsigned c, float mag) {   // -> mag * phasor
    const float p = __uint_as_float(c);
    const float q = 1.0f - fabsf(p);                                       // |Re| on the diamond |Re| + |Im| = 1
    const float xs = __uint_as_float(__float_as_uint(q) | (c << 31));
    const float g = mag * __builtin_amdgcn_rsqf(fmaf(p, p, q * q));       // 1/2 <= p^2 + q^2 <= 1
    return cmk(xs, p) * g;
}

// |S| x / |x|, and (|S|, 0) for a zero bin (numpy's exp(1j * angle(0)) = 1) WITHOUT a compare and two selects per bin: 1e-17 is
// added to the real part (a zero bin becomes (1e-17, 0) and normalises to (|S|, 0) within 5e-5; a bin of 1e-9 -- the spectrum
// X / 1024 of a frame at the -100 dB floor -- moves by 1e-8 of itself, below the rounding of the FFT that made it) and 1e-38 to
// |x|^2 (so that no reciprocal square root of zero is ever multiplied by zero).  6 VALU instructions per bin.
__device__ __forceinline__ cf gl_normalise(cf x, float mag) {
    const float xr = x.x + 1.0e-17f;
    const float s2 = fmaf(xr, xr, fmaf(x.y, x.y, 1.0e-38f));
    const float g = mag * __builtin_amdgcn_rsqf(s2);
    return cmk(xr, x.y) * g;
}
// The state of a bin between launches: the 32-bit phasor code (4 B in, 4 B out per bin and launch, 7 + 6 VALU instructions to
// decode / encode).  (Round 4 measured the raw spectrum value instead -- 8 B each way, decoded by the normalisation, encoded
// by nothing: the bytes cost more than the instructions, HISTORY.md part C; that build switch is in git history.)
typedef unsigned gl_state_t;
__device__ __forceinline__ gl_state_t gl_state_encode(cf x) { return gl_pack_phasor(x); }
__device__ __forceinline__ cf gl_state_decode(gl_state_t s, float mag) { return gl_unpack_phasor(s, mag); }
size_t gl_state_bytes() { return sizeof(gl_state_t); }

// ====================================================================================== streaming form
// One Griffin-Lim iteration (MODE 0) or the final iSTFT (MODE 1) WITHOUT phases: a run of consecutive frames of one
// utterance is a stream.  Frame index i of the run (frame t = run_t0 - halo + i, halo = ncol - 1) belongs to wave
// i mod 8, and a wave's iteration for index i is
//     decode + split + inverse FFT + synthesis window of frame i            (registers, the wave's exchange buffer)
//     overlap-add into a RING of R frames in LDS                            (in index order: a chain, see below)
//     forward FFT + merge + phasor code of frame i - halo                   (final once index i has been added)
// so loads of spectrum rows, arithmetic and stores of new rows interleave all the time instead of taking turns, no
// wave waits at a workgroup barrier inside a run (there is one per run), nothing is copied when the window moves on,
// and both windows stay in registers.  The eight waves drift apart by themselves (the chain staggers them), so the
// two waves of a SIMD are usually in different parts of the iteration.
//
// Ring.  A frame's SPAN is the 128-sample slots of its 2048 padded samples that the window touches (slots c_lo ..
// c_hi of the lane layout f = 2 (lane + 64 c) + e; 10 slots = 1280 samples for 1102): span sample q of index k lives
// at ring position hop (k mod R) + q.  The window is zero on the rest of the two outer slots, so whole slots are
// added (adding zeros) and no lane predicate is needed except in ONE slot: index k ACCUMULATES into span samples
// q < S - hop (what indices < k have written) and STORES the last hop samples (nobody has), so the ring is never
// cleared.  Spans that run past the end of the ring continue linearly into a GUARD of S - hop samples; the first
// index of the next lap (k mod R == 0) reads its accumulate part from the guard and writes it to the start of the
// ring (the guard is zeroed when a run starts: index 0 is such a fold, too).  Overlap-adds happen in index order --
// index i waits for the LDS word `ola_done` to reach i and sets it to i + 1 afterwards (LDS executes a wave's
// operations in order: the flag store follows the data stores) -- which fixes the summation order of every sample
// (bit-reproducible) and is the only synchronisation inside a run: once index i has been added, every frame <= i - halo
// has its final signal, and what the forward FFT of frame i - halo reads is not written again before the ring comes
// round (R >= 9 + halo + ceil(S / hop) + 1: by the time an index may overwrite a position, every wave has finished the
// iteration that read it; gl_stream_ring_frames).  The forward transform's input is read linearly, a ds_read2 and a packed
// multiply per slot.  A frame whose span crosses the end of the ring after the next lap has folded (the final values of the
// wrapped part are at the ring's start, not in the guard: ring slots sm with hop sm + S > hop R and R - sm <= lag, the last
// min(lag, ceil(S / hop) - 1) of every R frames -- 4 of 24 with three iterations per launch at 1102 / 275, 4 of 38 with two,
// 4 of 64 with one) reads its slots at or above the end ring_len lower and the one slot that straddles it element by element
// (fft_input).  Until round 7 those frames took the index-mapped path -- an address computation and a ds_read_b32 per sample,
// ~500 VALU instructions per frame against ~55 -- that only the frames whose window leaves the signal (reflect padding: 4 to
// 12 per utterance and iteration) need and take now.
// MODE 1 writes out, straight from the overlap-add's registers, the hop samples that index i makes final.
#define GL_NO_ITEM 0x7FFFFFFEu   // "not drawn yet" in the control word of the next item (item ids are < 2^31 - 2)
enum { CT_OLA = 0, CT_SNEXT = 1, CT_OLB = 2 /* chain words of stages 1, 2 */ };   // of the CT_SWORDS control words (gl_plan.h)

// NST = 2: TWO iterations per launch.  The kernel draws a constant amount of power per instruction and per byte, and
// with the spectra streaming the chip holds a shader clock of ~1.9 GHz against ~2.3 GHz for the same arithmetic without
// memory traffic (a shader-clock probe, round 6): what shortens the launch is energy, not overlap.  So the second iteration is fed
// from registers: stage A is the iteration above on ring A; its merged spectrum of frame t - lag is normalised to
// |S| e^{i phi} where it stands (no phasor code written, none read back: 8 instead of 12 bytes per bin and iteration,
// ~90 VALU instructions per frame and iteration less) and goes straight into stage B -- inverse FFT, overlap-add into
// ring B in the order of ITS chain, forward FFT of frame t - 2 lag, phasor code, store.  A run then needs halo + lag
// more frames at either end in stage A (2.6 % more transforms for runs of 144 frames).
// SEEDED: stage 0 makes its input from the seed (the first launch of a call without an initial-phase array) -- an
// instantiation of its own: as a run-time branch it cost every launch 38 more spilled registers.
// MOM: fast Griffin-Lim (Perraudin, Balazs, Soendergaard 2013).  The phasor code that leaves the launch is that of
// t = c + alpha (c - c_prev) instead of the projection c itself; c (the merged spectrum X / MH, 8 bytes per bin, float32: a
// 16-bit state does not hold the parity bound) goes to p.mom_c, from where the next iteration reads it as c_prev.  One
// iteration per launch only: the frames whose c a run reads and writes are then exactly the frames it owns (the halo frames
// of a run are decoded from their codes and transformed back, never projected), so the buffer is updated in place, no run
// reads what another writes and the cut does not reach the bits.  Fused stages would need stage k's c of a frame `lag`
// indices later in another wave: 8.2 KB per frame, a dozen frames per stage -- more than the rings leave of the LDS
// ("Fast Griffin-Lim").  The first iteration of a call (p.mom_first) has no c_prev: t = c, nothing is read.
// RAG: a ragged batch (tts_griffin_lim_ragged).  The frames of a run's utterance, Tb = p.n_frames[b], are loaded with the item
// (wave-uniform: a scalar) and take the place of p.T wherever the END of the utterance matters -- the row clamps, the interior
// test of the synthesis window, the signal length L of the reflect padding, `valid` / `emit` -- while p.T = T_max stays the
// stride of every buffer, so rows t >= Tb are never read.  1 / window sum-square at an utterance's ends comes from its own
// table (p.rw_edge); the interior image in registers does not depend on the length.  An instantiation of its own, as SEEDED
// and MOM are: with RAG = false Tb and L are the constants they were and the code is what it was ("Ragged
// Griffin-Lim", has the resource table).
template <int MODE, int WIN_CT, int HOP_CT, bool MSE, int NST = 1, bool SEEDED = false, bool MOM = false, bool RAG = false>
__global__ __launch_bounds__(GL_THREADS) void gl_stream_kernel(GlParams p) {
    static_assert(!SEEDED || MODE == 0, "the seeded start is an iteration's");
    static_assert(!MOM || (MODE == 0 && NST == 1), "momentum: one iteration per launch");
    static_assert(NST == 1 || (NST >= 2 && NST <= 3 && MODE == 0 && !MSE), "several iterations per launch: plain iterations only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int win = WIN_CT ? WIN_CT : p.win;
    const int hop = HOP_CT ? HOP_CT : p.hop;
    const int ncol = (WIN_CT && HOP_CT) ? (WIN_CT + HOP_CT - 1) / (HOP_CT ? HOP_CT : 1) : p.ncol;
    const int halo = ncol - 1;
    const int wpad = (NFFT - win) >> 1;
    const int c_lo = wpad >> 7;                        // first / last 128-sample slot the window touches
    const int c_hi = (wpad + win - 1) >> 7;
    // the same two as constants where the window is one: registers c < FZ_LO and c > FZ_HI of a forward transform's input
    // are zero (fft_input) and its first radix-16 leaves them out (fft16<ZLO, ZHI>); patterns it does not know: no pruning
    constexpr int fz_lo_ = WIN_CT ? ((NFFT - WIN_CT) >> 1) >> 7 : 0;
    constexpr int fz_hi_ = WIN_CT ? (((NFFT - WIN_CT) >> 1) + WIN_CT - 1) >> 7 : 15;
    constexpr bool fz_ok_ = fz_lo_ <= 4 && fz_hi_ >= 11 && fz_hi_ <= 15;
    constexpr int FZ_LO = fz_ok_ ? fz_lo_ : 0, FZ_HI = fz_ok_ ? fz_hi_ : 15;
    const int n_sl = c_hi - c_lo + 1;
    const int S = 128 * n_sl;                          // span of a frame in the ring
    const int fs = 128 * c_lo;                         // padded sample of span sample 0
    const int acc_len = S - hop;                       // span samples that earlier indices have written
    // A frame's forward FFT runs `lag` indices behind its overlap-add: halo, or one more when the reflect padding of the
    // signal's first frame reaches exactly as far as halo frames make final (windows with ncol * hop == win)
    const int lag = (halo + 1) * hop > 2 * (MH - wpad) ? halo : halo + 1;
    const int R = p.ring_frames;
    const int ring_len = hop * R;
    const int ring_floats = (ring_len + acc_len + 128 + 3) & ~3;
    const int L = hop * (p.T - 1);                     // samples of the (trimmed) signal; RAG: of a row of p.wav
    // RAG: frames and samples of the run's utterance, set per run (below); GL_TB / GL_L are p.T and L otherwise, the very
    // expressions the uniform kernel has always had
    int Tb_r = p.T;
    int L_r = L;
    const float* rw_head = nullptr;                    // RAG: 1 / window sum-square of the utterance's first / last rw_E samples,
    const float* rw_tail = nullptr;                    //      both based so that the padded sample index addresses them
#define GL_TB (RAG ? Tb_r : p.T)
#define GL_L (RAG ? L_r : L)
    // carve: [exchange: GL_NW * EX_CPLX cf][control][ring A: ring_len + acc_len + 128 floats][ring B]
    cf* ex_all = reinterpret_cast<cf*>(smem_raw);
    int* ctrl = reinterpret_cast<int*>(ex_all + GL_NW * EX_CPLX);
    float* ringA = reinterpret_cast<float*>(ctrl + CT_SWORDS);   // the ring of stage k follows at k * ring_floats

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // the wave index as a SCALAR: everything derived from it (frame index, ring slot, the branches on them) then lives
    // in SGPRs and branches without exec masks -- as `tid >> 6` it is a vector value to the compiler
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    cf* ex = ex_all + wave * EX_CPLX;

    // ---------------- one-time setup: twiddles and BOTH windows in registers
    if (tid == 0) ctrl[CT_SNEXT] = (int)atomicAdd(p.work_counter, 1u);
    // (the counter of the launch before this one on the stream is drained: every workgroup that drew from it has ended)
    if (tid == 0 && blockIdx.x == 0 && p.clear_counter) *p.clear_counter = 0u;
    // twr[j] = W2048^{lane + 64 j} for j < 8; W2048^{512} = -i, so slot j + 8 uses -i twr[j] (folded into the adds)
    cf twr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) twr[j] = reinterpret_cast<const cf*>(p.tw2048)[lane + 64 * j];
    FftTwReg tw;
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) tw.a[k2 - 1] = reinterpret_cast<const cf*>(p.tables)[1024 + (k2 - 1) * 64 + lane];
#pragma unroll
    for (int d = 1; d < 4; ++d) tw.b[d - 1] = reinterpret_cast<const cf*>(p.tw1024)[16 * (lane & 15) * d];
    // p.wlane: [set][lane][c][e], set 0 = analysis window w[n] / (2 MH), set 1 = set 0 / window-sum-square at an
    // interior frame (gl_build_wlane); zero outside the window, statically so for the slots outside the span
    float wana[16][2], wsyn[16][2];
    {
        const float4* wa = reinterpret_cast<const float4*>(p.wlane + (0 * 64 + lane) * 32);
        const float4* ws = reinterpret_cast<const float4*>(p.wlane + (1 * 64 + lane) * 32);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 a4 = wa[q], s4 = ws[q];
            wana[2 * q][0] = a4.x; wana[2 * q][1] = a4.y; wana[2 * q + 1][0] = a4.z; wana[2 * q + 1][1] = a4.w;
            wsyn[2 * q][0] = s4.x; wsyn[2 * q][1] = s4.y; wsyn[2 * q + 1][0] = s4.z; wsyn[2 * q + 1][1] = s4.w;
        }
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (WIN_CT && (c < c_lo || c > c_hi)) { wana[c][0] = wana[c][1] = wsyn[c][0] = wsyn[c][1] = 0.f; }
        // the inverse transform's output is conj(z): the sign of the odd sample is in the window, so that the synthesis window
        // is one packed multiply per pair (as `v * cmk(w0, -w1)` it was two scalar ones: the negation is not a source modifier
        // the compiler forms on a packed operand)
#pragma unroll
        for (int c = 0; c < 16; ++c) wsyn[c][1] = -wsyn[c][1];
    }
    __syncthreads();
    int item = __builtin_amdgcn_readfirstlane(ctrl[CT_SNEXT]);

    // ---------------- work item -> (utterance, first frame, frames, slot of its partial results); wave-uniform
    auto decode_item = [&](int it, int& b, int& t0, int& len, int& slot, int& tb) {
        const int4 q = p.items[it];   // (wave-uniform index: a scalar load)
        b = q.x; t0 = q.y; len = q.z; slot = q.w;
        if (RAG) tb = p.n_frames[q.x];   // (a scalar load as well)
    };

    // prefetch registers of one spectrum row in the pair-owner layout: phasor codes and magnitudes of bins lane + 64 j
    // (j < 8) and MH - lane - 64 (j - 8) (j >= 8), and of bin 512 (`nyq_*`: the name is older than the layout; only lane 0's is used)
    gl_state_t gc[16];
    float gs[16];
    gl_state_t nyq_c;
    float nyq_s;
    constexpr bool seeded = SEEDED;
#define GLS_LOAD_ROW(BASE_C, BASE_M, TF, TB)                                                    \
    {                                                                                           \
        int tf_ = (TF);                                                                         \
        tf_ = tf_ < 0 ? 0 : (tf_ >= (TB) ? (TB) - 1 : tf_);                                     \
        const gl_state_t* prow_ = (BASE_C) + (size_t)tf_ * p.FP;                                \
        const float* srow_ = (BASE_M) + (size_t)tf_ * p.FP;                                     \
        const gl_state_t* plo_ = prow_ + lane; const gl_state_t* phi_ = prow_ + (MH - lane);    \
        const float* slo_ = srow_ + lane; const float* shi_ = srow_ + (MH - lane);              \
        if (!seeded) {                                                                          \
            _Pragma("unroll") for (int j_ = 0; j_ < 16; ++j_) gc[j_] = GL_ROW(plo_, phi_, j_); \
            nyq_c = prow_[MH / 2];                                                              \
        }                                                                                       \
        _Pragma("unroll") for (int j_ = 0; j_ < 16; ++j_) gs[j_] = GL_STREAM_LOAD(j_ < 8 ? slo_ + 64 * j_ : shi_ - 64 * (j_ - 8)); \
        nyq_s = srow_[MH / 2];                                                                  \
    }
    // vmcnt counts loads and stores together, in issue order.  The row for the next iteration is requested early in
    // this one and the new row is stored at its end, so at the top of the loop the loads are OLDER than 17 stores: the
    // compiler's wait for "the last load" there (it does not carry the stores round the loop) is a wait for every store
    // of the previous iteration to reach memory -- a full write latency per iteration.  Touching the row registers just
    // before the stores makes the compiler wait for the loads there, where they are the youngest operations and some
    // microseconds old; at the top of the loop nothing is left to wait for (every path into the loop settles them).
#define GLS_TOUCH_ROW()                                                                                              \
    asm volatile("" : "+v"(gc[0]), "+v"(gc[1]), "+v"(gc[2]), "+v"(gc[3]), "+v"(gc[4]), "+v"(gc[5]), "+v"(gc[6]),       \
                      "+v"(gc[7]), "+v"(gc[8]), "+v"(gc[9]), "+v"(gc[10]), "+v"(gc[11]), "+v"(gc[12]), "+v"(gc[13]), \
                      "+v"(gc[14]), "+v"(gc[15]), "+v"(nyq_c));                                                      \
    asm volatile("" : "+v"(gs[0]), "+v"(gs[1]), "+v"(gs[2]), "+v"(gs[3]), "+v"(gs[4]), "+v"(gs[5]), "+v"(gs[6]),       \
                      "+v"(gs[7]), "+v"(gs[8]), "+v"(gs[9]), "+v"(gs[10]), "+v"(gs[11]), "+v"(gs[12]), "+v"(gs[13]), \
                      "+v"(gs[14]), "+v"(gs[15]), "+v"(nyq_s));
    const gl_state_t* x_in = reinterpret_cast<const gl_state_t*>(p.phase_in);
    gl_state_t* x_out = reinterpret_cast<gl_state_t*>(p.phase_out);

    // Issue priority by lateness.  The overlap-add chain makes every wave do one index per round; the hardware
    // arbitrates the two waves of a SIMD by age, so waves 0-3 run ahead, then sleep at the chain while their partners
    // (4-7) run alone -- and a wave alone on a SIMD fills fewer issue slots than two (the timeline showed 2.4 us of
    // waiting per 7.5 us iteration for the older half, none for the younger).  A wave whose next overlap-add is what the
    // chain will ask for next raises its priority, one that is far ahead lowers it: the waves then arrive at the chain
    // about when it is their turn.
#define GLS_URGENCY(NEXT_INDEX)                                                                    \
    {                                                                                              \
        const int d_ = __builtin_amdgcn_readfirstlane((NEXT_INDEX) - gl_flag_load(ctrl + CT_OLA)); \
        if (d_ <= 1) __builtin_amdgcn_s_setprio(3);                                                \
        else if (d_ <= 3) __builtin_amdgcn_s_setprio(2);                                           \
        else if (d_ <= 5) __builtin_amdgcn_s_setprio(1);                                           \
        else __builtin_amdgcn_s_setprio(0);                                                        \
    }

    // ---------------- the pieces of an iteration (all inlined; `v` is the wave's FFT register set)
    // G in the pair-owner layout (gk[c] = G[k], gk[8 + c] = G[MH - k], k = lane + 64 c; mid = G[512], lane 0's) -> input of
    // the inverse transform, v[j] = Zin[lane + 64 j] (real-FFT split pass): Zin[k] = conj(E + i O), Zin[MH-k] = E - i O with
    // E = G[k] + conj G[MH-k], O = conj(W^k) (G[k] - conj G[MH-k]) (the transform is fed conj(Zin), the two 1/2 are in the
    // window); the owner keeps Zin[k] and sends Zin[MH-k] to the lane that transforms it
    auto split_pass = [&](cf (&gk)[16], cf mid, cf (&v)[16]) __attribute__((always_inline)) {
        cf* wr = ex + (MH - lane);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            cf xk = gk[c];
            cf xm = gk[8 + c];
            if (c == 0 && lane == 0) { xk.y = 0.f; xm.y = 0.f; }   // DC and Nyquist bins are real
            const cf e = cadd_conj(xk, xm);
            const cf o = cmul_conj(csub_conj(xk, xm), twr[c]);
            v[c] = cconj_add_pi(e, o);
            wr[-64 * c] = cadd_mi(e, o);          // (lane 0, c = 0: slot MH, read by nobody)
        }
        if (lane == 0) ex[MH / 2] = cscale(mid, 2.0f);   // bin 512 is its own mirror: Zin = 2 G
        wave_lds_sync();
#pragma unroll
        for (int j = 8; j < 16; ++j) v[j] = ex[lane + 64 * j];
        wave_lds_sync();
    };
    // z[m] = conj(v) / MH, m = lane + 64 c: x[2m] = Re, x[2m+1] = Im; synthesis window (with 1 / window-sum-square)
    auto synth_window = [&](int t, cf (&v)[16]) __attribute__((always_inline)) {
        if (t >= halo && t + halo < GL_TB) {
#pragma unroll
            for (int c = 0; c < 16; ++c) v[c] = v[c] * cmk(wsyn[c][0], wsyn[c][1]);   // (wsyn[c][1] carries the conjugation's sign)
        } else {
            // frame near an utterance end: fewer overlapping neighbours, 1 / wss per sample (rare)
            const float* rwp = (RAG ? (t < halo ? rw_head : rw_tail) : p.rwss) + (size_t)t * hop + wpad;
#pragma unroll
            for (int c0 = 0; c0 < 16; c0 += 4) {
#pragma unroll
                for (int c = c0; c < c0 + 4; ++c) {
                    const int nw0 = 2 * (lane + 64 * c) - wpad;
                    const bool i0 = nw0 >= 0 && nw0 < win, i1 = nw0 + 1 >= 0 && nw0 + 1 < win;
                    const float r0 = rwp[i0 ? nw0 : 0], r1 = rwp[i1 ? nw0 + 1 : 0];
                    v[c] = cmk(i0 ? v[c].x * wana[c][0] * r0 : 0.f, i1 ? -v[c].y * wana[c][1] * r1 : 0.f);
                }
                asm volatile("" ::: "memory");
            }
        }
    };
    // overlap-add of index idx (ring slot s, frame t) into `ring`, in the order of the chain word `chain`
    float pk = 0.f;
    auto overlap_add = [&](float* ring, int chain, int idx, int s, int t, int b, int run_t0, int run_len, const cf (&v)[16])
                           __attribute__((always_inline)) {
        // Everything that does not depend on the ring comes BEFORE the wait for the chain: a chain step -- flag seen, reads,
        // adds, writes, flag passed on -- is what the eight waves of a workgroup do one after another (0.7 us per step in the
        // per-wave timeline; the final iSTFT, one stage per index, is bound by it), so the addresses and the masks of the
        // boundary slot are made while the wave would wait anyway, and what MODE 1 does with the finished samples (stores to
        // the waveform, the running peak) comes AFTER the flag is passed on.
        // Element (float) offsets of this lane's pair in span slot 0, for writing and for reading (the first index of a
        // lap folds the guard in).  One opaque base per PAIR of slots: slot 2k + 1 is 512 bytes behind slot 2k, which the
        // two 8-bit dword offsets of ds_read2 / ds_write2 reach (left to itself the compiler makes an address per slot and
        // direction: 18 VALU instructions per overlap-add).
        // (offsets from the start of the workgroup's LDS, not from `ring`: a stage's ring is a run-time base, and base +
        // constant + 512 is not folded into the instruction's offset fields)
        float* const lds_f = reinterpret_cast<float*>(smem_raw);
        const int e_wr = (int)(ring - lds_f) + hop * s + 2 * lane;
        const int e_rd = e_wr + (s == 0 ? ring_len : 0);
        int wo[8], ro[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            wo[k] = e_wr + 256 * k;
            ro[k] = e_rd + 256 * k;
            if (2 * k < n_sl) asm volatile("" : "+v"(wo[k]), "+v"(ro[k]));
        }
        // the slot where accumulate turns into store: which of this lane's two samples earlier indices have written
        const int qb_edge = 128 * ((acc_len - 1) >> 7);
        unsigned keep0 = qb_edge + 2 * lane < acc_len ? ~0u : 0u, keep1 = qb_edge + 2 * lane + 1 < acc_len ? ~0u : 0u;   // (bit masks)
        asm volatile("" : "+v"(keep0), "+v"(keep1));
        while (gl_flag_load(ctrl + chain) < idx) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
        cf fin[16];   // MODE 1: what the slots hold after this index (the finished samples are among them)
        {
            // All reads first, then the adds, then the writes: written slot by slot, every read waits for the
            // previous slot's write (the compiler cannot tell that they do not alias) and the critical section of
            // the chain is eight LDS round trips instead of one.
            cf o[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int j = c - c_lo;
                o[c] = cmk(0.f, 0.f);
                if (j < 0 || j >= n_sl) continue;                  // wave-uniform (static for the reference window)
                const int qb = 128 * j;
                const float* rp = lds_f + ro[j >> 1] + 128 * (j & 1);
                if (qb < acc_len) o[c] = cmk(rp[0], rp[1]);
            }
            asm volatile("" ::: "memory");
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int j = c - c_lo;
                if (j < 0 || j >= n_sl) continue;
                const int qb = 128 * j;
                cf a = v[c];                                       // a slot no earlier index has written: a plain store
                if (qb < acc_len) {
                    cf acc = o[c];
                    if (qb + 127 >= acc_len) {                     // (qb == qb_edge)
                        acc.x = __uint_as_float(__float_as_uint(acc.x) & keep0);
                        acc.y = __uint_as_float(__float_as_uint(acc.y) & keep1);
                    }
                    a = cadd(acc, v[c]);
                }
                float* wp = lds_f + wo[j >> 1] + 128 * (j & 1);
                wp[0] = a.x;
                wp[1] = a.y;
                if (MODE == 1) fin[c] = a;
            }
        }
        asm volatile("" ::: "memory");
        if (lane == 0) gl_flag_store(ctrl + chain, idx + 1);
        if (MODE == 1) {
            // span samples [q_fin, q_fin + hop) of this index are final now; y of span sample 0
            asm volatile("" ::: "memory");
            const int q_fin = wpad - fs;
            const int y0 = t * hop + fs - MH;
            const bool emit = (t >= run_t0 || run_t0 == 0) && (t < run_t0 + run_len || run_t0 + run_len == GL_TB);
            float* wb = p.wav + (size_t)b * L;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int j = c - c_lo;
                if (j < 0 || j >= n_sl) continue;
                const int qb = 128 * j;
                if (qb + 127 >= q_fin && qb < q_fin + hop) {       // slot holds final samples (wave-uniform)
                    const int q = qb + 2 * lane;
                    const int y = y0 + q;
                    const cf a = fin[c];
                    if (emit && q >= q_fin && q < q_fin + hop && y >= 0 && y < GL_L) { wb[y] = a.x; pk = fmaxf(pk, fabsf(a.x)); }
                    if (emit && q + 1 >= q_fin && q + 1 < q_fin + hop && y + 1 >= 0 && y + 1 < GL_L) { wb[y + 1] = a.y; pk = fmaxf(pk, fabsf(a.y)); }
                }
            }
        }
    };
    // windowed input of the forward transform of frame tm, whose overlap-add index was idx - lag (ring slot sm), read in
    // the iteration of index idx of its stage (y_base: trimmed-signal index of that stage's ring coordinate 0)
    auto fft_input = [&](const float* ring, int idx, int sm, int tm, int y_base, cf (&v)[16]) __attribute__((always_inline)) {
        const int ylo = tm * hop + wpad - MH;                    // y index of window sample 0
        const bool edge = ylo < 0 || ylo + win > GL_L;              // reflect padding needed
        // Three read paths.  LINEAR: the span does not cross the end of the ring, or the next lap's fold (index m + R - sm,
        // m = idx - lag) has not happened yet -- what it will fold is still in the guard, behind the ring.  WRAPPED LINEAR:
        // the span crosses the end and the fold has happened (R - sm <= lag): the final values of the wrapped part are at the
        // ring's start, so the span sample at ring position pos = hop sm + q is at pos below ring_len and at pos - ring_len
        // from there on.  Both are ONE loop: sm, hop and R are wave-uniform, so the 128-sample slots are classified with
        // scalars.  j_sel is the first slot that is not wholly below ring_len (past every slot on the linear path); the
        // pairs of slots from there on take their base ring_len lower, which is right for every slot wholly below and every
        // slot wholly at or above the end, and slot j_sel -- the only one that can straddle it, and with an odd hop one of
        // its pairs can, too -- is read again behind the loop, two ds_read_b32 with a compare and a select per address.
        // (What the loop read for that slot lies within the workgroup's LDS: at most 128 floats into the guard, or in front
        // of the ring, where the control words and the exchange buffers are.)  INDEX-MAPPED: reflect padding only.
        if (!edge) {
            // (one opaque LDS base per pair of slots, as in overlap_add; a packed multiply per slot)
            const float* const lds_f = reinterpret_cast<const float*>(smem_raw);
            const int pos0 = hop * sm;                               // ring position of span sample 0
            const int ring_e = (int)(ring - lds_f);
            const int e_rd = ring_e + pos0 + 2 * lane;
            const bool folded = pos0 + S > ring_len && R - sm <= lag;
            const int j_sel = folded ? (ring_len - pos0) >> 7 : 0x7fff;
            int ro[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ro[k] = e_rd + (256 * k - (2 * k >= j_sel ? ring_len : 0));
                if (2 * k < n_sl) asm("" : "+v"(ro[k]));
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int j = c - c_lo;
                if (j < 0 || j >= n_sl) { v[c] = cmk(0.f, 0.f); continue; }
                const float* sf = lds_f + ro[j >> 1] + 128 * (j & 1);
                v[c] = cmk(wana[c][0], wana[c][1]) * cmk(sf[0], sf[1]);
            }
            if (j_sel < n_sl) {
                const int q0 = pos0 + 128 * j_sel + 2 * lane;        // < ring_len + 128
                const int a0 = ring_e + (q0 >= ring_len ? q0 - ring_len : q0);
                const int a1 = ring_e + (q0 + 1 >= ring_len ? q0 + 1 - ring_len : q0 + 1);
                const cf x = cmk(lds_f[a0], lds_f[a1]);
                // (selects, not branches: as `if (c - c_lo == j_sel) v[c] = ...` this was a switch whose every case copied the
                // other slots' registers -- 380 instructions per call site for the 40 of a multiply and two selects per slot)
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    if (c < c_lo || c > c_hi) continue;
                    const cf y = cmk(wana[c][0], wana[c][1]) * x;
                    const bool hit = c - c_lo == j_sel;              // (wave-uniform)
                    v[c] = cmk(hit ? y.x : v[c].x, hit ? y.y : v[c].y);
                }
            }
        } else {
            // index-mapped reads: reflect at the signal's ends; run coordinate u = lap * ring_len + off lives at
            // ring position off -- unless off < acc_len and that lap's fold (index lap * R) is still to come:
            // then it is in the guard
            const int lap0 = (idx - lag) / R;
            const int ub = y_base + lap0 * ring_len;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                float x[2] = {0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int f = 2 * (lane + 64 * c) + e;
                    const int nw = f - wpad;
                    if (nw >= 0 && nw < win) {
                        int y = ylo + nw;
                        y = y < 0 ? -y : y;
                        y = y >= GL_L ? 2 * (GL_L - 1) - y : y;
                        int off = y - ub, lap = lap0;
                        if (off >= ring_len) { off -= ring_len; ++lap; }
                        else if (off < 0) { off += ring_len; --lap; }
                        const int pos = (off < acc_len && lap * R > idx) ? ring_len + off : off;
                        x[e] = wana[c][e] * ring[pos];
                    }
                }
                v[c] = cmk(x[0], x[1]);
            }
        }
    };
    // forward transform output (v[j] = Z[lane + 64 j], after fft1024) -> X / MH in the pair-owner layout (real-FFT merge pass):
    // sink(c, X[k]) and sink(8 + c, X[MH - k]) for k = lane + 64 c, c < 8; returns X[512] (meaningful in lane 0).  The upper
    // registers travel to their owners through the wave's exchange buffer; Z[MH] := Z[0] gives lane 0 its Nyquist bin.
    auto merge_pass = [&](const cf (&v)[16], auto&& sink) __attribute__((always_inline)) -> cf {
#pragma unroll
        for (int j = 8; j < 16; ++j) ex[lane + 64 * j] = v[j];
        if (lane == 0) ex[MH] = v[0];
        wave_lds_sync();
        cf zm[8];   // all mirrored values first: one LDS latency for the pass instead of one per pair
        const cf* rd = ex + (MH - lane);
#pragma unroll
        for (int c = 0; c < 8; ++c) zm[c] = rd[-64 * c];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const cf e = cadd_conj(v[c], zm[c]);
            const cf o = cmul(csub_conj(v[c], zm[c]), twr[c]);
            sink(c, cadd_mi(e, o));               // 2 X[k] = E - i o
            sink(8 + c, cconj_add_pi(e, o));      // 2 X[MH - k] = conj(E + i o)
        }
        wave_lds_sync();
        return cscale(cconj(v[8]), 2.0f);         // 2 X[512] = 2 conj(Z[512])
    };

    const int lead = NST * halo;   // frames the first index (of stage 0) lies before the run
    bool have_row = false;   // (per wave) the first row of this run was requested in the last iteration of the previous one
    while (item < p.n_items) {
        int b, run_t0, run_len, slot;
        decode_item(item, b, run_t0, run_len, slot, Tb_r);
        if (RAG) {
            L_r = hop * (Tb_r - 1);
            // the utterance's table: [first rw_E entries | last rw_E entries] of 1 / window sum-square at ITS length (whose
            // n_fft + L entries are fewer than rw_E where it has `halo` frames or less: both halves then start at entry 0)
            const int cut = NFFT + L_r - p.rw_E;
            rw_head = p.rw_edge + (size_t)b * 2 * p.rw_E;
            rw_tail = rw_head + p.rw_E - (cut > 0 ? cut : 0);
        }
        const float* magb = p.mag + (size_t)b * p.T * p.FP;
        const gl_state_t* phb = x_in + (size_t)b * p.T * p.FP;
        // The next item is drawn LATE in a run (by the wave of index n_idx - 24, read by every wave in its last iteration):
        // drawn at the start, a workgroup committed itself to a second run before it knew how long the first would take, and
        // a cut with runs of two lengths (gl_plan_items) paired long runs with short ones at random.  Runs too short for
        // that (fewer than four rounds of the waves) still draw it at the start.
        const int n_idx = run_len + NST * (halo + lag);
        const bool late = n_idx >= 4 * GL_NW;
        const int i_res = n_idx - 3 * GL_NW;
        unsigned next_item_reg = GL_NO_ITEM;
        if (tid == 0 && !late) next_item_reg = atomicAdd(p.work_counter, 1u);
        if (!have_row) GLS_LOAD_ROW(phb, magb, run_t0 - lead + wave, GL_TB)
        have_row = false;
        // run start: the guards read as zero for index 0, the chains start at 0
        for (int q = tid; q < acc_len + 128; q += GL_THREADS) {
#pragma unroll
            for (int k = 0; k < NST; ++k) ringA[k * ring_floats + ring_len + q] = 0.f;
        }
        if (tid == 0) { ctrl[CT_OLA] = 0; ctrl[CT_OLB] = 0; ctrl[CT_OLB + 1] = 0; ctrl[CT_SNEXT] = (int)next_item_reg; }
        __syncthreads();
        int next_item = __builtin_amdgcn_readfirstlane(ctrl[CT_SNEXT]);   // (late: GL_NO_ITEM until the wave's last iteration)
        int nb = b, nt0 = 0, nlen = 0, nslot = 0, nTb = p.T;
        if (!late && next_item < p.n_items) decode_item(next_item, nb, nt0, nlen, nslot, nTb);

        // the LAST stage (the only one of NST == 1) has the indices of one iteration, j <-> frame run_t0 - halo + j; every
        // stage before it runs halo + lag indices ahead of the next: stage 0 index i <-> frame run_t0 - NST halo + i
        const int y_base_a = (run_t0 - lead) * hop - MH + fs;   // trimmed-signal index of stage 0's ring coordinate 0 (lap 0)
        float mse_acc = 0.f;
        pk = 0.f;
        int s = wave % R;                                     // ring slot of this wave's index (wave < 8 <= R)
        GLS_TOUCH_ROW()
        for (int i = wave; i < n_idx; i += GL_NW) {
            const int t = run_t0 - lead + i;
            const bool valid = t >= 0 && t < GL_TB;           // wave-uniform
            unsigned drawn = 0;
            if (late && i == i_res && lane == 0) drawn = atomicAdd(p.work_counter, 1u);   // (consumed before this index's overlap-add)
            if (late && i + GL_NW >= n_idx) {
                // this wave's last iteration: its previous one waited for the chain to pass index i - 8 > i_res, whose wave
                // stored the item before it passed the chain on (LDS executes a wave's operations in order)
                int nv;
                while ((nv = gl_flag_load(ctrl + CT_SNEXT)) == (int)GL_NO_ITEM) __builtin_amdgcn_s_sleep(1);
                next_item = __builtin_amdgcn_readfirstlane(nv);
                if (next_item < p.n_items) decode_item(next_item, nb, nt0, nlen, nslot, nTb);
            }
            GLS_URGENCY(i)
            cf v[16];
            if (valid) {
                cf gk[16];   // X[k] = |S[k]| * phasor[k]
                if (seeded) {
                    const unsigned long long row0 = (unsigned long long)b * p.F * p.T + (unsigned long long)t;   // bin f: + f T
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const cf e = gl_seed_phasor(p.seed, row0 + (unsigned long long)GL_BIN(lane, j) * p.T);
                        gk[j] = cmk(gs[j] * e.x, gs[j] * e.y);
                    }
                    const cf en = gl_seed_phasor(p.seed, row0 + (unsigned long long)(MH / 2) * p.T);
                    split_pass(gk, cmk(nyq_s * en.x, nyq_s * en.y), v);
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j) gk[j] = gl_state_decode(gc[j], gs[j]);
                    split_pass(gk, gl_state_decode(nyq_c, nyq_s), v);
                }
            } else {
                // (zeros from asm statements: as constants the sixteen pairs are materialised in FRONT of the branch on
                // `valid` -- 32 v_mov in every iteration for the few indices that lie outside the utterance)
#pragma unroll
                for (int j = 0; j < 16; ++j) asm volatile("v_mov_b64 %0, 0" : "=v"(v[j]));
            }
            GLS_URGENCY(i)
            // the row is consumed.  NST == 1: request this wave's next one now (of this run, or the first of the next item).
            // NST > 1: the LAST stage requests it; the magnitude registers first take |S| of the frames that go from stage to
            // stage, each requested where its stage starts (below)
#define GLS_NEXT_ROW()                                                                                                   \
            if (i + GL_NW < n_idx) {                                                                                     \
                GLS_LOAD_ROW(phb, magb, t + GL_NW, GL_TB)                                                                \
            } else if (next_item < p.n_items) {                                                                          \
                GLS_LOAD_ROW(x_in + (size_t)nb * p.T * p.FP, p.mag + (size_t)nb * p.T * p.FP, nt0 - lead + wave, (RAG ? nTb : p.T)) \
                have_row = true;                                                                                         \
            }
            if (NST == 1) {
                GLS_NEXT_ROW()
            }
            if (valid) {
                fft1024(v, ex, tw, lane);
                synth_window(t, v);
            }
            if (late && i == i_res && lane == 0) gl_flag_store(ctrl + CT_SNEXT, (int)drawn);
            overlap_add(ringA, CT_OLA, i, s, t, b, run_t0, run_len, v);
            if (NST == 1) {
                // the next row has arrived (requested before the inverse FFT) -- settled on every path round the loop, at
                // the point of the iteration where the fewest registers are live, before this iteration's stores are issued
                GLS_TOUCH_ROW()
            }
            GLS_URGENCY(i + GL_NW)

            // ---------------- further stages: stage k runs halo + lag indices behind stage k - 1 and takes the forward
            // transform of stage k - 1's frame t_k = t_{k-1} - lag, normalised to |S| e^{i phi} in registers, as its input.
            // A loop, not NST copies of the code: the instruction cache is shared by two compute units.
            int sk = s, ik = i, tk = t;               // ring slot, index and frame of the current stage
            float* ring_k = ringA;
            int yb_k = y_base_a;
#pragma nounroll
            for (int k = 1; k < NST; ++k) {
                const int i_prev = ik, s_prev = sk;
                const float* ring_prev = ring_k;
                const int yb_prev = yb_k;
                ik -= halo + lag;
                tk -= lag;
                sk -= halo + lag;
                sk += sk < 0 ? R : 0;
                ring_k += ring_floats;
                yb_k += halo * hop;
                const bool valid_k = ik >= 0 && tk >= 0 && tk < GL_TB;
                {
                    // |S| of this stage's frame, requested where the stage starts (the forward transform covers the loads;
                    // unconditional: a row that is not needed is one that exists).  ONE load site for every further stage --
                    // round 6: requested at the end of the stage before, beside the last stage's request for the next row,
                    // the two sites' registers met in a phi, the allocator gave this site temporaries and copied them into
                    // place behind an `s_waitcnt vmcnt(1)` right after the loads (a whole memory round trip exposed per
                    // iteration), and because those temporaries were transform registers as well, the compiler's waits for
                    // "loads that may still write them" stood in the middle of the transforms and inside the overlap-add's
                    // critical section: 190.5 -> 185.9 us per iteration alone (profiles/r06_experiment_gl_issue.txt)
                    const int tq = tk < 0 ? 0 : (tk >= GL_TB ? GL_TB - 1 : tk);
                    const float* mrow_ = magb + (size_t)tq * p.FP;
                    const float* mlo_ = mrow_ + lane; const float* mhi_ = mrow_ + (MH - lane);
#pragma unroll
                    for (int j = 0; j < 16; ++j) gs[j] = GL_ROW(mlo_, mhi_, j);
                    nyq_s = mrow_[MH / 2];
                }
                if (valid_k) {
                    int sm = s_prev - lag;
                    sm += sm < 0 ? R : 0;
                    fft_input(ring_prev, i_prev, sm, tk, yb_prev, v);
                    fft1024<FZ_LO, FZ_HI>(v, ex, tw, lane);
                    cf gk[16];
                    // |S| e^{i phi}: x * (|S| / |x|), and (|S|, 0) for a zero bin (numpy's exp(1j * angle(0)) = 1); the
                    // bins are X / MH of a windowed signal, far from both ends of the float range
                    const cf xmid = merge_pass(v, [&](int c, cf x) { gk[c] = gl_normalise(x, gs[c]); });   // |S| e^{i phi}
                    split_pass(gk, gl_normalise(xmid, nyq_s), v);
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j) asm volatile("v_mov_b64 %0, 0" : "=v"(v[j]));   // (as in stage 0)
                }
                if (k + 1 == NST) {
                    GLS_NEXT_ROW()
                }
                if (ik >= 0) {
                    if (valid_k) {
                        fft1024(v, ex, tw, lane);
                        synth_window(tk, v);
                    }
                    overlap_add(ring_k, CT_OLB + k - 1, ik, sk, tk, b, run_t0, run_len, v);
                }
            }
            if (NST > 1) GLS_TOUCH_ROW()
            // ---------------- forward FFT of the frame `lag` behind in the last stage: its signal is final
            const int jj = ik, sb = sk;
            if (MODE == 0 && jj >= halo + lag && jj < halo + lag + run_len) {
                const int tm = tk - lag;                                 // in [run_t0, run_t0 + run_len), < T
                int sm = sb - lag;
                sm += sm < 0 ? R : 0;
                const float* mrow = magb + (size_t)tm * p.FP;
                float mg[16];
                if (MSE) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) mg[c] = fabsf(GL_STREAM_LOAD(c < 8 ? mrow + lane + 64 * c : mrow + (MH - lane) - 64 * (c - 8)));
                }
                // momentum: the previous projection of this frame, requested in front of the transform that covers the loads
                cf cp[16], cp_mid = cmk(0.f, 0.f);
                cf* const crow = MOM ? reinterpret_cast<cf*>(p.mom_c) + ((size_t)b * p.T + tm) * p.FP : nullptr;
                cf* const clo = MOM ? crow + lane : nullptr;
                cf* const chi = MOM ? crow + (MH - lane) : nullptr;
                const bool mom_prev = MOM && !p.mom_first;   // (a kernel argument: a scalar branch)
                if (MOM) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) cp[c] = cmk(0.f, 0.f);
                    if (mom_prev) {
#pragma unroll
                        for (int c = 0; c < 16; ++c) cp[c] = __builtin_nontemporal_load(c < 8 ? clo + 64 * c : chi - 64 * (c - 8));
                        cp_mid = crow[MH / 2];
                    }
                }
                // t = c + alpha (c - c_prev); the first iteration of a call: t = c
                auto mom_t = [&](cf x, cf prev) __attribute__((always_inline)) -> cf {
                    return mom_prev ? cadd(x, cscale(csub(x, prev), p.mom_alpha)) : x;
                };
                fft_input(ring_k, jj, sm, tm, yb_k, v);
                fft1024<FZ_LO, FZ_HI>(v, ex, tw, lane);
                GLS_URGENCY(i + GL_NW)
                // momentum: the squared error goes out per FRAME (p.mse_partial [B][T], summed in frame order by the reduction), so
                // that the mse, like the waveform, is the same bits whatever runs the frames lie in
                if (MOM && MSE) mse_acc = 0.f;
                gl_state_t* orow = x_out + ((size_t)b * p.T + tm) * p.FP;
                gl_state_t* olo = orow + lane;
                gl_state_t* ohi = orow + (MH - lane);
                const cf xmid = merge_pass(v, [&](int c, cf x) {
                    if (MOM) {
                        GL_STREAM_STORE(c < 8 ? clo + 64 * c : chi - 64 * (c - 8), x);
                        __builtin_nontemporal_store(gl_state_encode(mom_t(x, cp[c])), c < 8 ? olo + 64 * c : ohi - 64 * (c - 8));
                    } else
                    __builtin_nontemporal_store(gl_state_encode(x), c < 8 ? olo + 64 * c : ohi - 64 * (c - 8));
                    if (MSE) {
                        const float d = mg[c] - (float)MH * sqrtf(fmaf(x.x, x.x, x.y * x.y));   // x = X / MH
                        mse_acc += d * d;
                    }
                });
                if (lane == 0) {
                    if (MOM) crow[MH / 2] = xmid;
                    __builtin_nontemporal_store(gl_state_encode(MOM ? mom_t(xmid, cp_mid) : xmid), orow + MH / 2);   // bin 512
                    if (MSE) {
                        const float d = fabsf(mrow[MH / 2]) - (float)MH * sqrtf(fmaf(xmid.x, xmid.x, xmid.y * xmid.y));
                        mse_acc += d * d;
                    }
                }
                if (MOM && MSE) {
                    float r = mse_acc;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o);
                    if (lane == 0) p.mse_partial[(size_t)b * p.T + tm] = r;
                }
            }
            s += GL_NW;
            s -= s >= R ? R : 0;
        }
        __builtin_amdgcn_s_setprio(0);
        // ---------------- run end: per-run partial results (fixed order), then everyone is done with the rings
        if ((MODE == 0 && MSE && !MOM) || (MODE == 1 && p.peak_partial)) {
            float r = MODE == 0 ? mse_acc : pk;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) r = MODE == 0 ? r + __shfl_xor(r, o) : fmaxf(r, __shfl_xor(r, o));
            __syncthreads();   // all waves are done with their exchange buffers
            float* red = reinterpret_cast<float*>(ex_all);
            if (lane == 0) red[wave] = r;
            __syncthreads();
            if (tid == 0) {
                float a = 0.f;
                for (int w = 0; w < GL_NW; ++w) a = MODE == 0 ? a + red[w] : fmaxf(a, red[w]);
                float* part = (MODE == 0 ? p.mse_partial : p.peak_partial) + (size_t)b * p.slots_per_utt + (slot & 0xffff);
                part[0] = a;
                for (int q = 1; q <= (slot >> 16); ++q) part[q] = 0.f;   // (the utterance's last run: slots other utterances have)
            }
        }
        __syncthreads();
        item = next_item;
    }
#undef GLS_LOAD_ROW
#undef GL_TB
#undef GL_L
#undef GLS_NEXT_ROW
#undef GLS_TOUCH_ROW
#undef GLS_URGENCY
}

// ---- streaming form: launch (geometry and the cut of a batch into runs: gl_plan.hip)

// The (window, hop) pairs the streaming kernel is instantiated for (both windows in registers, every span bound static): the
// model's 50 ms / 12.5 ms at the reference's 22.05 kHz (1102 / 275, dataset_params.sampling_rate; audio/conversion.py:122-136)
// and, round 6, the same 50 / 12.5 ms at 16 kHz (800 / 200).  Any other pair takes the general kernels of
// griffin_lim_generic.hip.  The run-time (WIN_CT = HOP_CT = 0) form of the kernel body stays in the source for the tools; it
// needed ~100 spilled registers per lane.
bool gl_stream_instantiated(int win, int hop) { return (win == 1102 && hop == 275) || (win == 800 && hop == 200); }

// THE table of launch forms: the kernel that runs (final iSTFT, with the mse, iterations per launch, seeded start, momentum),
// null where there is none.  What is configured and what is launched are both read from it.  RAG: the ragged instantiations
// (p.n_frames set) -- the same forms, one for one.
typedef void (*GlStreamKernel)(GlParams);
template <int W, int H, bool RAG>
static GlStreamKernel gl_stream_form_wh(bool final_istft, bool mse, int n_stage, bool seeded, bool mom) {
    if (final_istft) return (mse || n_stage != 1 || seeded || mom) ? nullptr : &gl_stream_kernel<1, W, H, false, 1, false, false, RAG>;
    if (mom) {
        // one iteration per launch: plain, seeded (a call's first launch) and with the mse (its last); a call with momentum has
        // at least two iterations, so no launch is seeded AND asked for the mse
        if (n_stage != 1 || (mse && seeded)) return nullptr;
        if (mse) return &gl_stream_kernel<0, W, H, true, 1, false, true, RAG>;
        return seeded ? &gl_stream_kernel<0, W, H, false, 1, true, true, RAG> : &gl_stream_kernel<0, W, H, false, 1, false, true, RAG>;
    }
    if (mse)   // (the last iteration of a call, alone in its launch)
        return n_stage != 1 ? nullptr : seeded ? &gl_stream_kernel<0, W, H, true, 1, true, false, RAG> : &gl_stream_kernel<0, W, H, true, 1, false, false, RAG>;
    switch (n_stage) {
        case 1: return seeded ? &gl_stream_kernel<0, W, H, false, 1, true, false, RAG> : &gl_stream_kernel<0, W, H, false, 1, false, false, RAG>;
        case 2: return seeded ? &gl_stream_kernel<0, W, H, false, 2, true, false, RAG> : &gl_stream_kernel<0, W, H, false, 2, false, false, RAG>;
        case 3: return seeded ? &gl_stream_kernel<0, W, H, false, 3, true, false, RAG> : &gl_stream_kernel<0, W, H, false, 3, false, false, RAG>;
    }
    return nullptr;
}
static GlStreamKernel gl_stream_form(int win, int hop, bool rag, bool final_istft, bool mse, int n_stage, bool seeded, bool mom) {
    if (win == 1102 && hop == 275)
        return rag ? gl_stream_form_wh<1102, 275, true>(final_istft, mse, n_stage, seeded, mom) : gl_stream_form_wh<1102, 275, false>(final_istft, mse, n_stage, seeded, mom);
    if (win == 800 && hop == 200)
        return rag ? gl_stream_form_wh<800, 200, true>(final_istft, mse, n_stage, seeded, mom) : gl_stream_form_wh<800, 200, false>(final_istft, mse, n_stage, seeded, mom);
    return nullptr;
}

// p.work_counter must point at a zeroed counter that no other launch uses; p.items: a table of gl_plan_items.
// n_stage = 2, 3: that many iterations in this launch (phase_in -> phase_out is then SEVERAL Griffin-Lim iterations); not for
// the final iSTFT, not with the mse and not with momentum.
hipError_t launch_gl_stream(hipStream_t s, const GlParams& p_in, int n_cus, int final_istft, int n_stage) {
    GlParams p = p_in;
    p.n_stage = n_stage;
    if (n_stage < 1 || n_stage > 3) return hipErrorInvalidValue;
    p.ring_frames = gl_stream_ring_frames(p.win, p.hop, n_stage);
    if (p.ring_frames < GL_NW) return hipErrorInvalidValue;
    if (p.n_frames && (!p.rw_edge || p.rw_E != gl_rw_edge_len(NFFT, p.win, p.hop))) return hipErrorInvalidValue;
    // (the final iSTFT of a call with momentum is the plain one)
    const GlStreamKernel kernel = gl_stream_form(p.win, p.hop, p.n_frames != nullptr, final_istft != 0, p.mse_partial != nullptr, n_stage,
                                                 p.seeded != 0, p.mom_c && !final_istft);
    if (!kernel) return hipErrorInvalidValue;
    // one workgroup per compute unit (256 registers x 8 waves), as many as the cut was made for
    const int nwg = p.n_workers > 0 && p.n_workers < n_cus ? p.n_workers : (p.n_items < n_cus ? p.n_items : n_cus);
    hipLaunchKernelGGL(kernel, dim3(nwg), dim3(GL_THREADS), gl_stream_lds_bytes(p.win, p.hop, p.ring_frames, n_stage), s, p);
    return hipGetLastError();
}

// every launch form of every instantiation may take the whole LDS budget: the table's whole domain, walked once
static hipError_t gl_stream_configure() {
    for (int wh = 0; wh < 2; ++wh)
        for (int rag = 0; rag < 2; ++rag)
            for (int i = 0; i < 16 * 3; ++i) {   // four flags and 1..3 iterations per launch
                const bool final_istft = i & 1, mse = i & 2, seeded = i & 4, mom = i & 8;
                const GlStreamKernel kernel = gl_stream_form(wh ? 800 : 1102, wh ? 200 : 275, rag, final_istft, mse, 1 + i / 16, seeded, mom);
                if (!kernel) continue;
                const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GL_LDS_BUDGET);
                if (e != hipSuccess) return e;
            }
    return hipSuccess;
}

// ------------------------------------------------------------------------------------ analysis STFT
// librosa.stft(center=True, reflect, hann) of real signals: one wave per frame, signal read straight
// from global memory (this is the feature-extraction side, reference audio/features.py:62,145 --
// not part of the synthesis loop).  out [B][Tf][FP] complex.
__global__ __launch_bounds__(GL_THREADS) void stft_kernel(const float* __restrict__ wav, int n, int Tf,
                                                          const float* __restrict__ window, int win, int hop,
                                                          const cf* __restrict__ tw1024, const cf* __restrict__ tw2048,
                                                          cf* __restrict__ out, int FP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* ex_all = reinterpret_cast<cf*>(smem_raw);
    cf* twR = ex_all + GL_NW * EX_CPLX;
    cf* twA = twR + 1024;
    float* wtab = reinterpret_cast<float*>(twA + 15 * 64);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cf* ex = ex_all + wave * EX_CPLX;
    for (int i = tid; i < win; i += GL_THREADS) wtab[i] = window[i];
    for (int i = tid; i < 1024; i += GL_THREADS) twR[i] = tw2048[i];
    for (int i = tid; i < 15 * 64; i += GL_THREADS) twA[i] = tw1024[(i & 63) * ((i >> 6) + 1)];
    FftTw tw;
#pragma unroll
    for (int d = 1; d < 4; ++d) tw.b[d - 1] = tw1024[16 * (lane & 15) * d];
    tw.a = twA + lane;
    __syncthreads();
    const int b = blockIdx.y;
    const int t = blockIdx.x * GL_NW + wave;
    if (t >= Tf) return;
    const float* y = wav + (size_t)b * n;
    const int wpad = (NFFT - win) >> 1;
    const int ylo = t * hop + wpad - MH;
    cf v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int nn = 2 * (lane + 64 * j);
        float x[2] = {0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int nw = nn + e - wpad;
            if (nw >= 0 && nw < win) {
                int yi = ylo + nw;
                yi = yi < 0 ? -yi : yi;
                yi = yi >= n ? 2 * (n - 1) - yi : yi;
                x[e] = wtab[nw] * y[yi];
            }
        }
        v[j] = cmk(x[0], x[1]);
    }
    fft1024(v, ex, tw, lane);
#pragma unroll
    for (int c = 0; c < 16; ++c) ex[lane + 64 * c] = v[c];
    wave_lds_sync();
    cf* orow = out + ((size_t)b * Tf + t) * FP;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int k = lane + 64 * c;
        const cf zk = v[c];
        const cf zr = ex[(MH - k) & (MH - 1)];
        const cf e = cscale(cadd_conj(zk, zr), 0.5f);
        const cf o = cmul(cscale(csub_conj(zk, zr), 0.5f), twR[k]);
        orow[k] = cadd_mi(e, o);
    }
    if (lane == 0) orow[MH] = cmk(v[0].x - v[0].y, 0.f);
    if (lane < FP - MH - 1) orow[MH + 1 + lane] = cmk(0.f, 0.f);
}

static hipError_t stft_configure() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&stft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GL_LDS_BUDGET);
}
// Function attributes are per device: called once per handle (on the handle's device) by api_stages.hip.
hipError_t gl_configure() {
    const hipError_t e = gl_stream_configure();
    return e != hipSuccess ? e : stft_configure();
}

hipError_t launch_stft(hipStream_t s, const float* wav, int B, int n, int Tf, const float* window, int win, int hop,
                       const float2* tw1024, const float2* tw2048, float2* out, int FP) {
    const size_t lds = (size_t)(GL_NW * EX_CPLX + 1024 + 15 * 64) * sizeof(cf) + (size_t)((win + 3) & ~3) * sizeof(float);
    dim3 grid((Tf + GL_NW - 1) / GL_NW, B);
    hipLaunchKernelGGL(stft_kernel, grid, dim3(GL_THREADS), lds, s, wav, n, Tf, window, win, hop,
                       reinterpret_cast<const cf*>(tw1024), reinterpret_cast<const cf*>(tw2048), reinterpret_cast<cf*>(out), FP);
    return hipGetLastError();
}

// complex (B,T,FP) -> (B,F,T): mode 0 interleaved complex64, mode 1 |z| ** power
__global__ void cplx_tf_to_ft_kernel(const cf* in, float* out, int F, int T, int FP, int mode, float power) {
    __shared__ cf tile[32][33];
    const int b = blockIdx.z;
    const int f0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, f = f0 + tx;
        tile[i][tx] = (t < T && f < F) ? in[((size_t)b * T + t) * FP + f] : cmk(0.f, 0.f);
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int f = f0 + i, t = t0 + tx;
        if (f < F && t < T) {
            const cf z = tile[tx][i];
            const size_t o = ((size_t)b * F + f) * T + t;
            if (mode == 0) {
                reinterpret_cast<cf*>(out)[o] = z;
            } else {
                const float m = sqrtf(z.x * z.x + z.y * z.y);
                out[o] = power == 1.0f ? m : (power == 2.0f ? m * m : powf(m, power));
            }
        }
    }
}
hipError_t launch_cplx_tf_to_ft(hipStream_t s, const float2* in, float* out, int B, int F, int T, int FP, int mode,
                                float power) {
    dim3 grid((T + 31) / 32, (F + 31) / 32, B);
    hipLaunchKernelGGL(cplx_tf_to_ft_kernel, grid, dim3(32, 8), 0, s, reinterpret_cast<const cf*>(in), out, F, T, FP, mode, power);
    return hipGetLastError();
}

// elementwise dB conversions of reference audio/conversion.py: mode 0 magnitude_to_decibel (:5-29),
// 1 decibel_to_magnitude (:32-53), 2 normalize_decibel (:56-78), 3 inv_normalize_decibel (:81-102)
__global__ void db_convert_kernel(const float* in, float* out, size_t n, int mode, float ref_db, float max_db) {
    const float range = fabsf(ref_db) + fabsf(max_db);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float x = in[i];
        float y;
        // np.maximum / np.clip hand a NaN on where fmaxf / fminf drop it: modes 0, 2 and 3 select it back (clip_keep_nan)
        if (mode == 0) y = (float)(20.0 * log10((double)(x != x ? x : fmaxf(1e-5f, x))));   // analysis side: exact rounding
        else if (mode == 1) y = exp2f(x * (0.05f * 3.3219280948873623f));
        else if (mode == 2) y = clip_keep_nan(1.0f + (x - ref_db) / range, 0.f, 1.f);
        else y = (clip_keep_nan(x, 0.f, 1.f) - 1.0f) * range + ref_db;
        out[i] = y;
    }
}
hipError_t launch_db_convert(hipStream_t s, const float* in, float* out, size_t n, int mode, float ref_db, float max_db) {
    const unsigned blocks = (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(db_convert_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, in, out, n, mode, ref_db, max_db);
    return hipGetLastError();
}

// any value below lim?  (decibel_to_magnitude's assertion, reference audio/conversion.py:47-49)
__global__ void any_below_kernel(const float* in, size_t n, float lim, int* flag) {
    bool hit = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        hit |= in[i] < lim;
    if (hit) *flag = 1;
}
hipError_t launch_any_below(hipStream_t s, const float* in, size_t n, float lim, int* flag) {
    const unsigned blocks = (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(any_below_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, in, n, lim, flag);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------ small kernels
// mse[b] = sum(partials[b][:]) / (F*T), fixed order.
__global__ void gl_mse_reduce_kernel(const float* partial, int nchunks, float denom, float* mse) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < nchunks; ++i) s += partial[(size_t)b * nchunks + i];
        mse[b] = s / denom;
    }
}
hipError_t launch_gl_mse_reduce(hipStream_t s, const float* partial, int B, int nchunks, float denom, float* mse) {
    hipLaunchKernelGGL(gl_mse_reduce_kernel, dim3(B), dim3(64), 0, s, partial, nchunks, denom, mse);
    return hipGetLastError();
}

// ragged: the utterance's own denominator F * n_frames[b], made as the uniform call makes its one (double product, then float);
// per_frame (momentum, general kernels): the row holds one partial per frame and the first n_frames[b] are summed, in frame
// order -- the sum of the single-utterance call, bit for bit.  Otherwise every slot of the row (the last run zeroed the unused)
__global__ void gl_mse_reduce_ragged_kernel(const float* partial, int nchunks, int F, const int* n_frames, int per_frame, float* mse) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        const int Tb = n_frames[b];
        const int n = per_frame ? Tb : nchunks;
        float s = 0.f;
        for (int i = 0; i < n; ++i) s += partial[(size_t)b * nchunks + i];
        mse[b] = s / (float)((double)F * Tb);
    }
}
hipError_t launch_gl_mse_reduce_ragged(hipStream_t s, const float* partial, int B, int nchunks, int F, const int* n_frames, int per_frame,
                                       float* mse) {
    hipLaunchKernelGGL(gl_mse_reduce_ragged_kernel, dim3(B), dim3(64), 0, s, partial, nchunks, F, n_frames, per_frame, mse);
    return hipGetLastError();
}

// (B,F,T) reference layout -> internal (B,T,FP) magnitude (abs taken, as griffin_lim_v2 does)
// RAG (a ragged batch): columns t >= n_frames[b] are neither read nor written; a tile that lies behind the utterance's end leaves
template <bool RAG>
__global__ void mag_ft_to_tf_kernel(const float* in, float* out, int F, int T, int FP, const int* n_frames) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int f0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;   // 32 x 8
    const int Tb = RAG ? n_frames[b] : T;
    if (RAG && t0 >= Tb) return;   // (the whole workgroup)
    for (int i = ty; i < 32; i += 8) {
        const int f = f0 + i, t = t0 + tx;
        tile[i][tx] = (f < F && t < Tb) ? fabsf(in[((size_t)b * F + f) * T + t]) : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, f = f0 + tx;
        if (t < Tb && f < FP) out[((size_t)b * T + t) * FP + f] = tile[tx][i];
    }
}
hipError_t launch_mag_ft_to_tf(hipStream_t s, const float* in, float* out, int B, int F, int T, int FP, const int* n_frames) {
    dim3 grid((T + 31) / 32, (FP + 31) / 32, B);
    if (n_frames) hipLaunchKernelGGL(mag_ft_to_tf_kernel<true>, grid, dim3(32, 8), 0, s, in, out, F, T, FP, n_frames);
    else hipLaunchKernelGGL(mag_ft_to_tf_kernel<false>, grid, dim3(32, 8), 0, s, in, out, F, T, FP, n_frames);
    return hipGetLastError();
}

// internal (B,T,FP) -> (B,F,T)
__global__ void tf_to_ft_kernel(const float* in, float* out, int F, int T, int FP) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int f0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, f = f0 + tx;
        tile[i][tx] = (t < T && f < F) ? in[((size_t)b * T + t) * FP + f] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int f = f0 + i, t = t0 + tx;
        if (f < F && t < T) out[((size_t)b * F + f) * T + t] = tile[tx][i];
    }
}
hipError_t launch_tf_to_ft(hipStream_t s, const float* in, float* out, int B, int F, int T, int FP) {
    dim3 grid((T + 31) / 32, (F + 31) / 32, B);
    hipLaunchKernelGGL(tf_to_ft_kernel, grid, dim3(32, 8), 0, s, in, out, F, T, FP);
    return hipGetLastError();
}

// angles = exp(2 pi i u): u from init (B,F,T) reference layout, or the seeded start (gl_seed_phasor: only needed as codes when
// no iteration follows -- the first launch of an iteration makes it itself); out (B,T,FP) phasor codes (no magnitudes
// needed: the state is the phasor alone).  Running it on a side stream beside the post-net was tried and cost 1.3 ms
// per step instead of saving 0.17: a third busy stream slows the Griffin-Lim launches of the main one.
// RAG (a ragged batch): as mag_ft_to_tf_kernel -- nothing behind n_frames[b] is read or written
template <bool RAG>
__global__ void phase_init_kernel(const float* init_ft, uint64_t seed, gl_state_t* out, int F, int T, int FP, const int* n_frames) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int f0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int Tb = RAG ? n_frames[b] : T;
    if (RAG && t0 >= Tb) return;   // (the whole workgroup)
    for (int i = ty; i < 32; i += 8) {
        const int f = f0 + i, t = t0 + tx;
        float u = 0.f;
        if (f < F && t < Tb) {
            const size_t idx = ((size_t)b * F + f) * T + t;
            u = init_ft ? init_ft[idx] : 0.f;
        }
        tile[i][tx] = u;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, f = f0 + tx;
        if (t < Tb && f < FP) {
            float sn, cs;
            sincospif(2.0f * tile[tx][i], &sn, &cs);
            cf e = cmk(cs, sn);   // phasor of exp(2 pi i u)
            if (!init_ft) e = f < F ? gl_seed_phasor(seed, ((unsigned long long)b * F + f) * T + t) : cmk(1.f, 0.f);   // the seeded start
            out[((size_t)b * T + t) * FP + f] = gl_state_encode(e);
        }
    }
}
hipError_t launch_phase_init(hipStream_t s, const float* init_ft, uint64_t seed, void* out, int B, int F, int T, int FP, const int* n_frames) {
    dim3 grid((T + 31) / 32, (FP + 31) / 32, B);
    if (n_frames) hipLaunchKernelGGL(phase_init_kernel<true>, grid, dim3(32, 8), 0, s, init_ft, seed, reinterpret_cast<gl_state_t*>(out), F, T, FP, n_frames);
    else hipLaunchKernelGGL(phase_init_kernel<false>, grid, dim3(32, 8), 0, s, init_ft, seed, reinterpret_cast<gl_state_t*>(out), F, T, FP, n_frames);
    return hipGetLastError();
}

// linear (B,T,F) network output -> internal magnitude (B,T,FP):
//   db = (clip(x,0,1) - 1) * (|ref| + |max|) + ref;  mag = 10^(db/20);  mag ** power
// below_flag (optional): set when some value de-normalises to less than -100 dB (decibel_to_magnitude's
// assertion, reference audio/conversion.py:47-49)
__global__ void denorm_power_kernel(const float* lin, float* mag, size_t rows, int F, int FP, float ref_db,
                                    float range_db, float power, int* below_flag) {
    const size_t row = blockIdx.x;
    if (row >= rows) return;
    const float* in = lin + row * F;
    float* out = mag + row * FP;
    bool below = false;
    for (int f = threadIdx.x; f < FP; f += blockDim.x) {
        float v = 0.f;
        if (f < F) {
            const float db = denorm_db(in[f], ref_db, range_db);
            below |= db < -100.0f;
            v = db_pow(db, power);
        }
        out[f] = v;
    }
    if (below_flag && below) *below_flag = 1;
}
hipError_t launch_denorm_power(hipStream_t s, const float* lin, float* mag, size_t rows, int F, int FP,
                               float ref_db, float max_db, float power, int* below_flag) {
    hipLaunchKernelGGL(denorm_power_kernel, dim3((unsigned)rows), dim3(256), 0, s, lin, mag, rows, F, FP, ref_db,
                       fabsf(ref_db) + fabsf(max_db), power, below_flag);
    return hipGetLastError();
}

// peak normalisation: wav /= max|wav| per utterance unless the peak is below FLT_MIN
__global__ __launch_bounds__(1024) void peak_normalize_kernel(float* wav, int n) {
    __shared__ float red[16];
    float* w = wav + (size_t)blockIdx.x * n;
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, fabsf(w[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) m = fmaxf(m, red[i]);
    if (m < 1.17549435e-38f) m = 1.0f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) w[i] = w[i] / m;
}
// wav /= max(partials[b][:]) (unless below FLT_MIN): second half of the fused peak normalisation
__global__ void peak_scale_kernel(float* wav, int n, const float* partial, int nparts) {
    const int b = blockIdx.y;
    float m = 0.f;
    for (int i = 0; i < nparts; ++i) m = fmaxf(m, partial[(size_t)b * nparts + i]);
    if (m < 1.17549435e-38f) m = 1.0f;
    float* w = wav + (size_t)b * n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) w[i] = w[i] / m;
}
hipError_t launch_peak_scale(hipStream_t s, float* wav, int B, int n, const float* partial, int nparts) {
    hipLaunchKernelGGL(peak_scale_kernel, dim3(64, B), dim3(256), 0, s, wav, n, partial, nparts);
    return hipGetLastError();
}

hipError_t launch_peak_normalize(hipStream_t s, float* wav, int B, int n) {
    hipLaunchKernelGGL(peak_normalize_kernel, dim3(B), dim3(1024), 0, s, wav, n);
    return hipGetLastError();
}

}  // namespace tts
