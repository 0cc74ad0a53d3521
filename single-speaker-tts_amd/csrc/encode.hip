// The delivery encoder (no reference counterpart): float32 rows to 16-bit PCM, 8-bit PCM, G.711 mu-law or A-law in one streaming
// pass.  include/sstts_hip.h has the definition in full and encode_plan.h the per-sample function, which is what runs here: the
// codes and the records are the bits of tests/encode_oracle.py.
//
//   enc_init_kernel   the records as a row without a sample has them: zeros and n
//   encode_kernel     a workgroup per tile of ENC_TILE samples of a row.  The groups of four samples whose codes start at an
//                     address aligned to four codes take one 16-byte load (four 4-byte loads where the caller's rows are not
//                     aligned alike) and one packed store of 8 or 4 bytes; the at most three samples in front of a tile's first
//                     such group and behind its last go one by one.  Samples at or behind a row's length are not read: their
//                     codes are the format's silence.  A lane counts its clipped and NaN samples and keeps its largest |q|; the
//                     wave's sums and maximum go to the row's record with integer atomics, which do not depend on the order.
// The lengths travel by value; no floating-point atomics.
#include "api_internal.h"
#include "encode_plan.h"

// v + d is one rounded sum (x * Q is exact either way); the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

struct EncLens {
    int n[ENC_UTTS];
};

template <int FMT>
struct EncCodeType {
    using type = unsigned char;
};
template <>
struct EncCodeType<ENC_S16> {
    using type = unsigned short;
};

__global__ void enc_init_kernel(tts_encode_stats_t* __restrict__ stats, EncLens lens, int nb) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    stats[b].clipped = 0;
    stats[b].nans = 0;
    stats[b].peak = 0;
    stats[b].n = lens.n[b];
}

// wav, out: the first row of the CALL, rows N elements apart; row blockIdx.y of the launch is row b0 + blockIdx.y of the call
// (the dither is a function of the call's row index); stats: the launch's records, initialised before.
template <int FMT, int DITHER>
__global__ __launch_bounds__(ENC_LANES) void encode_kernel(const float* __restrict__ wav, void* __restrict__ out_, size_t N, EncLens lens, int b0,
                                                           unsigned long long seed, tts_encode_stats_t* __restrict__ stats) {
    using code_t = typename EncCodeType<FMT>::type;
    using pack_t = typename std::conditional<FMT == ENC_S16, uint2, unsigned>::type;
    const int r = blockIdx.y, tid = threadIdx.x;
    const unsigned b = (unsigned)(b0 + r);
    const long long n = lens.n[r];
    const long long lo = (long long)blockIdx.x * ENC_TILE;
    const long long hi = lo + ENC_TILE < (long long)N ? lo + ENC_TILE : (long long)N;
    if (lo >= hi) return;
    const float* x = wav + (size_t)b * N;
    code_t* y = reinterpret_cast<code_t*>(out_) + (size_t)b * N;
    constexpr unsigned silence = enc_silence(FMT);
    EncCount c;

    // [lo, g0): one by one; [g0, g1): whole groups whose codes are aligned for a packed store; [g1, hi): one by one
    const int head = enc_head((unsigned long long)(reinterpret_cast<uintptr_t>(y + lo) / sizeof(code_t)));
    const long long g0 = lo + head < hi ? lo + head : hi;
    const long long groups = (hi - g0) / ENC_GROUP;
    const long long g1 = g0 + groups * ENC_GROUP;
    if (tid < ENC_GROUP - 1) {
        const long long i = lo + tid;
        if (i < g0) y[i] = (code_t)(i < n ? enc_sample(x[i], FMT, DITHER, seed, b, (uint32_t)i, c) : silence);
        const long long j = g1 + tid;
        if (j < hi) y[j] = (code_t)(j < n ? enc_sample(x[j], FMT, DITHER, seed, b, (uint32_t)j, c) : silence);
    }
    const bool wide = (reinterpret_cast<uintptr_t>(x + g0) & 15) == 0;   // (uniform over the tile)
    // (ENC_ROUNDS rounds of the lanes at most.  Issuing a lane's loads of all rounds ahead of the first encoding was measured and
    //  gained nothing: 0.061 against 0.056 ms at 64 x 275 000 samples)
    for (long long g = tid; g < groups; g += ENC_LANES) {
        const long long i = g0 + g * ENC_GROUP;
        unsigned q[ENC_GROUP] = {silence, silence, silence, silence};
        if (i + ENC_GROUP <= n) {
            float v[ENC_GROUP];
            if (wide) {
                const float4 f = *reinterpret_cast<const float4*>(x + i);
                v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
            } else {
#pragma unroll
                for (int u = 0; u < ENC_GROUP; ++u) v[u] = x[i + u];
            }
#pragma unroll
            for (int u = 0; u < ENC_GROUP; ++u) q[u] = enc_sample(v[u], FMT, DITHER, seed, b, (uint32_t)(i + u), c);
        } else if (i < n) {   // (the group the row's length cuts)
#pragma unroll
            for (int u = 0; u < ENC_GROUP; ++u)
                if (i + u < n) q[u] = enc_sample(x[i + u], FMT, DITHER, seed, b, (uint32_t)(i + u), c);
        }
        pack_t p;
        if constexpr (FMT == ENC_S16) {
            p.x = q[0] | (q[1] << 16);
            p.y = q[2] | (q[3] << 16);
        } else {
            p = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        }
        *reinterpret_cast<pack_t*>(y + i) = p;
    }

    if (lo >= n) return;   // (uniform: a tile of padding counts nowhere)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        c.clipped += __shfl_xor(c.clipped, off, 64);
        c.nans += __shfl_xor(c.nans, off, 64);
        const int o = __shfl_xor(c.peak, off, 64);
        if (o > c.peak) c.peak = o;
    }
    if ((tid & 63) == 0) {
        if (c.clipped) atomicAdd(&stats[r].clipped, c.clipped);
        if (c.nans) atomicAdd(&stats[r].nans, c.nans);
        if (c.peak) atomicMax(&stats[r].peak, c.peak);
    }
}

}  // namespace tts

namespace tts_api {

// The workspace of a tts_encode call on B rows whose caller takes no records.
int encode_scratch(tts_handle_t h, int B, EncScratch* s) {
    WS(h, "enc.stats", tts_encode_stats_t, (size_t)B, st);
    *s = EncScratch{st};
    return TTS_OK;
}

template <int FMT>
static void encode_launch(int dither, dim3 grid, hipStream_t stream, const float* wav, void* out, size_t N, const EncLens& lens, int b0, uint64_t seed,
                          tts_encode_stats_t* stats) {
    if (dither == ENC_DITHER_TPDF)
        hipLaunchKernelGGL((encode_kernel<FMT, ENC_DITHER_TPDF>), grid, dim3(ENC_LANES), 0, stream, wav, out, N, lens, b0, (unsigned long long)seed, stats);
    else
        hipLaunchKernelGGL((encode_kernel<FMT, ENC_DITHER_NONE>), grid, dim3(ENC_LANES), 0, stream, wav, out, N, lens, b0, (unsigned long long)seed, stats);
}

// On h->stream; everything has been checked (encode_check).
int encode_impl(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, int format, int dither, uint64_t seed, void* out,
                tts_encode_stats_t* stats) {
    tts_encode_stats_t* st = stats;
    if (!st) {
        EncScratch s;
        const int rc = encode_scratch(h, B, &s);
        if (rc) return rc;
        st = s.stats;
    }
    ProfScope ps(h, ST_ENCODE, (int64_t)length_chunks(B, ENC_UTTS) * 2);
    for (int b0 = 0; b0 < B; b0 += ENC_UTTS) {
        const int nb = std::min(ENC_UTTS, B - b0);
        EncLens lens;
        fill_lengths(lens.n, n_samples, b0, nb, N);
        const dim3 grid((unsigned)enc_tiles(N), nb);
        hipLaunchKernelGGL(enc_init_kernel, dim3(1), dim3(ENC_UTTS), 0, h->stream, st + b0, lens, nb);
        switch (format) {
            case ENC_S16: encode_launch<ENC_S16>(dither, grid, h->stream, wav, out, (size_t)N, lens, b0, seed, st + b0); break;
            case ENC_U8: encode_launch<ENC_U8>(dither, grid, h->stream, wav, out, (size_t)N, lens, b0, seed, st + b0); break;
            case ENC_MULAW: encode_launch<ENC_MULAW>(dither, grid, h->stream, wav, out, (size_t)N, lens, b0, seed, st + b0); break;
            default: encode_launch<ENC_ALAW>(dither, grid, h->stream, wav, out, (size_t)N, lens, b0, seed, st + b0); break;
        }
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_encode_width(int format) { return enc_width(format); }

int tts_encode_tile(void) { return ENC_TILE; }

int tts_encode(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, int format, int dither, uint64_t seed, void* out,
               tts_encode_stats_t* stats) {
    DeviceScope dev_scope(h);
    std::string why = encode_check(wav && out, B, N, n_samples, format, dither);
    if (why.empty() && (((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(stats)) & 3) ||
                        (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(enc_width(format) - 1))))
        why = "wav and stats must be 4-byte aligned, out as its codes are";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "encode: " + why);
    if (!h) return TTS_ERR_INVALID;
    return encode_impl(h, wav, B, N, n_samples, format, dither, seed, out, stats);
}

int tts_set_output(tts_handle_t h, int format, int dither, int rate_in, int rate_out) {
    if (!h) return TTS_ERR_INVALID;
    bool on = false;
    const std::string why = output_check(format, dither, rate_in, rate_out, &on);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "set_output: " + why);
    auto& o = h->settings.out;
    o.enabled = on;
    o.format = format;
    o.dither = format == ENC_F32 ? ENC_DITHER_NONE : dither;
    o.ratio = rate_in != rate_out ? (double)rate_out / (double)rate_in : 1.0;
    return TTS_OK;
}

}  // extern "C"
