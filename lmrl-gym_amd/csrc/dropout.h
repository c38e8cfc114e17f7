// dropout.h — the ONE definition of the train step's dropout keep masks, compiled for host and device like threefry.h.
//
// HF-Flax GPT-2 (transformers 4.26.1, 3rd party) drops at three kinds of site when `train=True`: the embedding output (`embd_pdrop`), the attention
// probabilities (`attn_pdrop`) and the outputs of the two `c_proj` products of a block (`resid_pdrop`), each with `jax.random.bernoulli(rng, 1 - p,
// shape)` and `x / (1 - p)` on the kept elements (flax.linen.Dropout / dot_product_attention_weights).  The masks here follow that draw's PUBLISHED
// algorithm on a key schedule of our own (jax is absent from the tree; flax's per-module key folding is not reproduced — DESIGN.md section 2):
//   * a forward call takes a key K = (k0, k1);
//   * site s uses K_s = threefry2x32_20(K, (0, s)) — jax.random.fold_in(K, s); s = 0 the embedding output, 1 + 3 l the attention probabilities of
//     block l, 2 + 3 l the attention c_proj output of block l, 3 + 3 l the MLP c_proj output of block l;
//   * element i is the row-major index into the site's logical tensor of n elements ([B, T, d], or [B, H, T, T] for the probabilities), n < 2^32;
//   * keep iff bitcast((jax_random_word(K_s, i, n) >> 9) | 0x3F800000) - 1.0f < 1 - p in fp32 (jax.random.uniform < p_keep), kept values times
//     1 / (1 - p).
// The float u = m 2^-23 with the 23-bit integer m = word >> 9, and (1 - p) 2^23 is exact in fp32, so u < 1 - p  <=>  m < ceil((1 - p) 2^23): the
// kernels compare integers (dropout_threshold).  Masks are never stored: the backward sweeps and the gradient-checkpointing recompute call the same
// functions with the same (K_s, i, n).
#pragma once
#include "threefry.h"

namespace lmrl {

struct DropoutSite {
    uint32_t k0, k1;     // K_s
    uint32_t n, h;       // elements of the site's tensor, ceil(n / 2) (the half split of jax's random_bits)
    uint32_t thr;        // keep iff (word >> 9) < thr
    float scale;         // 1 / (1 - p) in fp32
};

LMRL_TF_FN uint32_t dropout_threshold(float p) {
    const float keep = 1.0f - p;
    const float x = keep * 8388608.0f;            // exact: a power-of-two scale
    uint32_t t = (uint32_t)x;
    if ((float)t < x) t++;
    return t;
}

LMRL_TF_FN DropoutSite dropout_site(uint32_t k0, uint32_t k1, uint32_t site, uint32_t n, float p) {
    DropoutSite s;
    threefry2x32_20(k0, k1, 0u, site, s.k0, s.k1);
    s.n = n; s.h = (n + 1u) >> 1;
    s.thr = dropout_threshold(p);
    s.scale = 1.0f / (1.0f - p);
    return s;
}

// jax_random_word without the divergent branch (every lane runs one block function)
LMRL_TF_FN uint32_t dropout_word(const DropoutSite &s, uint32_t i) {
    const bool lo = i < s.h;
    const uint32_t c0 = lo ? i : i - s.h;
    const uint32_t c1 = lo ? ((i + s.h < s.n) ? i + s.h : 0u) : i;
    uint32_t y0, y1;
    threefry2x32_20(s.k0, s.k1, c0, c1, y0, y1);
    return lo ? y0 : y1;
}

LMRL_TF_FN bool dropout_keep(const DropoutSite &s, uint32_t i) { return (dropout_word(s, i) >> 9) < s.thr; }

// elements j < h and j + h of one site come out of ONE block function (words y0 and y1): the elementwise kernels walk the tensor in such pairs
LMRL_TF_FN void dropout_keep_pair(const DropoutSite &s, uint32_t j, bool &keep_lo, bool &keep_hi) {
    uint32_t y0, y1;
    threefry2x32_20(s.k0, s.k1, j, (j + s.h < s.n) ? j + s.h : 0u, y0, y1);
    keep_lo = (y0 >> 9) < s.thr;
    keep_hi = (y1 >> 9) < s.thr;
}

}  // namespace lmrl
