// The move of a tile of EQ_TILE_SEGS segments between a row in memory and LDS, shared by the stages that cut a row into EQ_SEG-sample
// segments and give a lane a segment (equalizer.hip, compressor.hip): the tile travels in 16-byte accesses of neighbouring lanes and
// lies in LDS in rows EQ_LDS_STRIDE floats apart (equalizer.hip has the bank arithmetic).  Device code: included by .hip files only.
#pragma once
#include "equalizer_plan.h"
#include <cstdint>

namespace tts {

constexpr int EQ_LANES = 64;
static_assert(EQ_LANES == EQ_TILE_SEGS, "a lane owns a segment of the tile");

// Samples [first, first + count) of the row x <-> the tile in LDS.  Whole 16-byte groups inside the range move as one access,
// the samples of a group that the range cuts one by one: nothing outside the range is touched.
template <bool LOAD>
__device__ __forceinline__ void eq_move_tile(float* x, long long first, int count, float* tile, int lane) {
    float* p = x + first;
    const int lead = (int)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);   // floats in front of the first aligned address
    // group g holds tile samples 4 g - (4 - lead) % 4 ... : shift so that group boundaries are 16-byte aligned addresses
    const int shift = (4 - lead) & 3;                    // samples of group 0 that lie in front of the range
    const int groups = (count + shift + 3) >> 2;
    for (int g = lane; g < groups; g += EQ_LANES) {
        const int e0 = 4 * g - shift;                    // the tile sample of the group's first float
        if (e0 >= 0 && e0 + 4 <= count) {
            float4* q = reinterpret_cast<float4*>(p + e0);
            if (LOAD) {
                const float4 v = *q;
                tile[((e0 + 0) >> 8) * EQ_LDS_STRIDE + ((e0 + 0) & (EQ_SEG - 1))] = v.x;
                tile[((e0 + 1) >> 8) * EQ_LDS_STRIDE + ((e0 + 1) & (EQ_SEG - 1))] = v.y;
                tile[((e0 + 2) >> 8) * EQ_LDS_STRIDE + ((e0 + 2) & (EQ_SEG - 1))] = v.z;
                tile[((e0 + 3) >> 8) * EQ_LDS_STRIDE + ((e0 + 3) & (EQ_SEG - 1))] = v.w;
            } else {
                float4 v;
                v.x = tile[((e0 + 0) >> 8) * EQ_LDS_STRIDE + ((e0 + 0) & (EQ_SEG - 1))];
                v.y = tile[((e0 + 1) >> 8) * EQ_LDS_STRIDE + ((e0 + 1) & (EQ_SEG - 1))];
                v.z = tile[((e0 + 2) >> 8) * EQ_LDS_STRIDE + ((e0 + 2) & (EQ_SEG - 1))];
                v.w = tile[((e0 + 3) >> 8) * EQ_LDS_STRIDE + ((e0 + 3) & (EQ_SEG - 1))];
                *q = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = e0 + j;
                if (e >= 0 && e < count) {
                    float* t = tile + (e >> 8) * EQ_LDS_STRIDE + (e & (EQ_SEG - 1));
                    if (LOAD)
                        *t = p[e];
                    else
                        p[e] = *t;
                }
            }
        }
    }
}

}  // namespace tts
