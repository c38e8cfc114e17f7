// embed_stats_core.h — one row of the LN-folded path's embedding (the body of embed_stats_kernel, csrc/gpt2.hip), shared with the fused
// reduce + accept + embed launch of the Wordle rollout.  One wave per row; d <= 64 * 4 * MAXV.
#pragma once
#include "gemm_bf16.h"

namespace lmrl {

// xr = te + pe (fp32), xbr = bf16(xr), stats slot 0 = (sum x, sum x^2), the other slots 0
template <int MAXV>
__device__ __forceinline__ void embed_stats_row(const uint16_t *__restrict__ te, const uint16_t *__restrict__ pe, float *__restrict__ xr,
                                                uint16_t *__restrict__ xbr, float2 *__restrict__ stats_r, int nslots, int d, int lane) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < MAXV; k++) {
        const int c = (k * 64 + lane) * 4;
        if (c < d) {
            const uint2 a = *reinterpret_cast<const uint2 *>(te + c), p = *reinterpret_cast<const uint2 *>(pe + c);
            const f32x4 v = f32x4{bf16_to_f32((uint16_t)(a.x & 0xffff)) + bf16_to_f32((uint16_t)(p.x & 0xffff)),
                                  bf16_to_f32((uint16_t)(a.x >> 16)) + bf16_to_f32((uint16_t)(p.x >> 16)),
                                  bf16_to_f32((uint16_t)(a.y & 0xffff)) + bf16_to_f32((uint16_t)(p.y & 0xffff)),
                                  bf16_to_f32((uint16_t)(a.y >> 16)) + bf16_to_f32((uint16_t)(p.y >> 16))};
            *reinterpret_cast<f32x4 *>(xr + c) = v;
            uint2 o;
            o.x = pack_bf16x2(v[0], v[1]);
            o.y = pack_bf16x2(v[2], v[3]);
            *reinterpret_cast<uint2 *>(xbr + c) = o;
            s1 += (v[0] + v[1]) + (v[2] + v[3]);
            s2 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    for (int sl = lane; sl < nslots; sl += 64) stats_r[sl] = sl == 0 ? make_float2(s1, s2) : make_float2(0.f, 0.f);
}

}  // namespace lmrl
