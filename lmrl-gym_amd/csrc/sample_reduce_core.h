// sample_reduce_core.h — merge of one row's per-tile sampling partials (the body of sample_reduce_kernel, csrc/sampler.hip), shared with the
// fused reduce + accept + embed launch of the Wordle rollout (csrc/gpt2.hip).  One wave per row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lmrl {

constexpr int kPartialFloats = 6;       // {max, sumexp, best_score, best_col, best_z, pad}
constexpr int kPartialTileCols = 128;   // vocabulary columns per partial (= the LM-head tile width kLmBN)

// token = argmax best_score ; logprob = best_z - logsumexp(z).  Lane 0 writes token[m] (and logprob[m]); an inactive row gets
// (pad_token, 0).  Returns the row's token on every lane that matters to the caller (lane 0).  `active` may alias memory the
// caller writes afterwards (the fused launch clears gen_active behind this read): no __restrict__ on it.
__device__ __forceinline__ int sample_reduce_row(const float *__restrict__ partials, const uint8_t *active, int32_t *__restrict__ token,
                                                 float *__restrict__ logprob, int m, int np, int pad_token, int lane) {
    if (active && !active[m]) {
        if (lane == 0) { token[m] = pad_token; if (logprob) logprob[m] = 0.f; }
        return pad_token;
    }
    float pmax = -INFINITY, psum = 0.f, best = -INFINITY, best_z = 0.f;
    int best_col = 0x7fffffff;
    for (int t = lane; t < np; t += 64) {
        const float *p = partials + ((size_t)m * np + t) * kPartialFloats;
        const float om = p[0], os = p[1], ob = p[2], oz = p[4];
        const int oc = __float_as_int(p[3]);
        const float nm = fmaxf(pmax, om);
        const float e1 = (pmax == -INFINITY) ? 0.f : __expf(pmax - nm), e2 = (om == -INFINITY) ? 0.f : __expf(om - nm);
        psum = psum * e1 + os * e2; pmax = nm;
        if (ob > best || (ob == best && oc < best_col)) { best = ob; best_col = oc; best_z = oz; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float om = __shfl_xor(pmax, o), os = __shfl_xor(psum, o), ob = __shfl_xor(best, o), oz = __shfl_xor(best_z, o);
        const int oc = __shfl_xor(best_col, o);
        const float nm = fmaxf(pmax, om);
        const float e1 = (pmax == -INFINITY) ? 0.f : __expf(pmax - nm), e2 = (om == -INFINITY) ? 0.f : __expf(om - nm);
        psum = psum * e1 + os * e2; pmax = nm;
        if (ob > best || (ob == best && oc < best_col)) { best = ob; best_col = oc; best_z = oz; }
    }
    if (lane == 0) {
        token[m] = best_col;
        if (logprob) logprob[m] = best_z - (pmax + __logf(psum));
    }
    return best_col;
}

}  // namespace lmrl
