// kv_prefix_f32.hip — the prompt-prefix cache of the fp32 rollout mode (GPT2EngineF32): the fp32 twins of gpt2.hip's kv_gather_kernel and
// kv_attach_kernel.
//
// A text env whose observations form a finite set (Maze with last_k = 1: one prompt per (goal, cell), llm_rl_scripts/maze/env/env.py:8-81)
// prefills every distinct prompt ONCE per set of weights into a prefix session (one cache row per prompt).  A turn then starts either with a copy
// of that row into every env's own cache (lmrl_kv_gather_f32) or with a pointer to it (lmrl_kv_attach_f32: the decode attention reads the
// prompt positions from the prefix row itself, lmrl_attn_decode_prefixed_f32 in csrc/attn_cached_f32.hip).
//
// Cache layout (KVSessionF32.kv): fp32 [n_layer][K|V][B][tmax][d]; per env also the last hidden state (ln_f of the last token) and the last
// residual before ln_f, both fp32 [B][d].
#include "../../include/lmrl_amd.h"
#include "common.h"

namespace lmrl {

// One workgroup per (env, layer x K|V), one float4 per lane and step.  idx[b] < 0 or out of range: the env gets an empty cache.  Rows at and beyond
// the copied length are not written.
__global__ __launch_bounds__(256) void kv_gather_f32_kernel(const float *__restrict__ src, int src_b, int src_tmax, const int32_t *__restrict__ src_len,
                                                            const int32_t *__restrict__ idx, float *__restrict__ dst, int dst_tmax, int B, int d,
                                                            const float *__restrict__ src_hidden, const float *__restrict__ src_last_x,
                                                            float *__restrict__ dst_hidden, float *__restrict__ dst_last_x, int32_t *__restrict__ dst_len) {
    const int b = blockIdx.x, lk = blockIdx.y;
    const int r = idx[b];
    const int n_pos = (r >= 0 && r < src_b) ? min(min(src_len[r], dst_tmax), src_tmax) : 0;
    if (n_pos > 0) {
        const float4 *sp = reinterpret_cast<const float4 *>(src + ((size_t)lk * src_b + r) * src_tmax * d);
        float4 *dp = reinterpret_cast<float4 *>(dst + ((size_t)lk * B + b) * dst_tmax * d);
        const int chunks = n_pos * d / 4;
        for (int i = threadIdx.x; i < chunks; i += blockDim.x) dp[i] = sp[i];
    }
    if (lk == 0) {
        if (n_pos > 0)
            for (int i = threadIdx.x; i < d / 4; i += blockDim.x) {
                if (dst_hidden) reinterpret_cast<float4 *>(dst_hidden + (size_t)b * d)[i] = reinterpret_cast<const float4 *>(src_hidden + (size_t)r * d)[i];
                if (dst_last_x) reinterpret_cast<float4 *>(dst_last_x + (size_t)b * d)[i] = reinterpret_cast<const float4 *>(src_last_x + (size_t)r * d)[i];
            }
        if (threadIdx.x == 0) dst_len[b] = n_pos;
    }
}

// Blocks [0, B): per-env bookkeeping — the cache length and the prefix length become the prompt length of row idx[b] (0 without a row), and the
// row's last hidden state / last residual are copied; nothing else.  Block B: the launch order, envs grouped by prefix row (a counting sort over
// the rows; the order inside a group only decides which waves run side by side).  Envs without a row are sorted last.
constexpr int kAttachMaxRowsF32 = 12288;     // prefix rows the LDS histogram holds (48 KB); more rows: identity order
__global__ __launch_bounds__(1024) void kv_attach_f32_kernel(int src_b, int src_tmax, const int32_t *__restrict__ src_len, const int32_t *__restrict__ idx,
                                                             int B, int d, int dst_tmax, const float *__restrict__ src_hidden,
                                                             const float *__restrict__ src_last_x, float *__restrict__ dst_hidden,
                                                             float *__restrict__ dst_last_x, int32_t *__restrict__ dst_len, int32_t *__restrict__ pfx_n,
                                                             int32_t *__restrict__ order) {
    const int b = blockIdx.x;
    if (b < B) {
        const int r = idx[b];
        const int n = (r >= 0 && r < src_b) ? min(min(src_len[r], dst_tmax), src_tmax) : 0;
        if (n > 0)
            for (int i = threadIdx.x; i < d / 4; i += blockDim.x) {
                if (dst_hidden) reinterpret_cast<float4 *>(dst_hidden + (size_t)b * d)[i] = reinterpret_cast<const float4 *>(src_hidden + (size_t)r * d)[i];
                if (dst_last_x) reinterpret_cast<float4 *>(dst_last_x + (size_t)b * d)[i] = reinterpret_cast<const float4 *>(src_last_x + (size_t)r * d)[i];
            }
        if (threadIdx.x == 0) { dst_len[b] = n; pfx_n[b] = n; }
        return;
    }
    if (!order) return;
    if (src_b > kAttachMaxRowsF32) {
        for (int i = threadIdx.x; i < B; i += blockDim.x) order[i] = i;
        return;
    }
    __shared__ int32_t hist[kAttachMaxRowsF32 + 1];
    __shared__ int32_t part[1024];
    const int nb = src_b + 1;                                // bucket src_b: envs without a prefix
    for (int i = threadIdx.x; i < nb; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        const int r = idx[i];
        atomicAdd(&hist[(r >= 0 && r < src_b) ? r : src_b], 1);
    }
    __syncthreads();
    // exclusive scan of the histogram: each thread owns a contiguous stretch of buckets
    const int per = (nb + blockDim.x - 1) / blockDim.x, lo = min((int)threadIdx.x * per, nb), hi = min(lo + per, nb);
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += hist[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < (int)blockDim.x; i++) { const int v = part[i]; part[i] = run; run += v; }
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; i++) { const int v = hist[i]; hist[i] = run; run += v; }
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        const int r = idx[i];
        order[atomicAdd(&hist[(r >= 0 && r < src_b) ? r : src_b], 1)] = i;
    }
}

// Beam search (lmrl_kv_reorder_f32, the fp32 twin of gpt2.hip's kv_reorder_kernel): row i of the destination cache continues source row
// parent[i] — K and V of the generated positions [from[i], src_len[parent[i]]) of every layer, the cache length, the last hidden state and the
// last residual.  Positions below from[i] (the attached prompt prefix) are not touched.  Out of place; *go == 0: nothing is written.
__global__ __launch_bounds__(256) void kv_reorder_f32_kernel(const float *__restrict__ src, const int32_t *__restrict__ src_len, const int32_t *__restrict__ parent,
                                                             const int32_t *__restrict__ from, float *__restrict__ dst, int32_t *__restrict__ dst_len, int B,
                                                             int tmax, int d, const float *__restrict__ src_hidden, const float *__restrict__ src_last_x,
                                                             float *__restrict__ dst_hidden, float *__restrict__ dst_last_x, const int32_t *__restrict__ go) {
    if (go && *go == 0) return;
    const int b = blockIdx.x, lk = blockIdx.y;
    const int r = parent[b];
    if (r < 0 || r >= B) return;
    const int hi = min(src_len[r], tmax), lo = min(max(from ? from[b] : 0, 0), hi);
    const float4 *sp = reinterpret_cast<const float4 *>(src + (((size_t)lk * B + r) * tmax + lo) * d);
    float4 *dp = reinterpret_cast<float4 *>(dst + (((size_t)lk * B + b) * tmax + lo) * d);
    const int chunks = (hi - lo) * (d / 4);
    for (int i = threadIdx.x; i < chunks; i += blockDim.x) dp[i] = sp[i];
    if (lk == 0) {
        for (int i = threadIdx.x; i < d / 4; i += blockDim.x) {
            if (dst_hidden) reinterpret_cast<float4 *>(dst_hidden + (size_t)b * d)[i] = reinterpret_cast<const float4 *>(src_hidden + (size_t)r * d)[i];
            if (dst_last_x) reinterpret_cast<float4 *>(dst_last_x + (size_t)b * d)[i] = reinterpret_cast<const float4 *>(src_last_x + (size_t)r * d)[i];
        }
        if (threadIdx.x == 0) dst_len[b] = hi;
    }
}

}  // namespace lmrl

using namespace lmrl;

extern "C" {

int lmrl_kv_gather_f32(const float *src_kv_d, int src_b, int src_tmax, const int32_t *src_len_d, const float *src_hidden_d, const float *src_last_x_d,
                       const int32_t *idx_d, float *dst_kv_d, int dst_tmax, int b, float *dst_hidden_d, float *dst_last_x_d, int32_t *dst_len_d,
                       int n_layer, int d, void *stream) {
    LMRL_REQUIRE(src_kv_d && src_len_d && idx_d && dst_kv_d && dst_len_d && b > 0 && src_b > 0 && src_tmax > 0 && dst_tmax > 0 && n_layer > 0 &&
                 d > 0 && d % 4 == 0, "lmrl_kv_gather_f32: bad argument");
    LMRL_REQUIRE((!dst_hidden_d || src_hidden_d) && (!dst_last_x_d || src_last_x_d), "lmrl_kv_gather_f32: a destination row without its source");
    hipLaunchKernelGGL(kv_gather_f32_kernel, dim3(b, 2 * n_layer), dim3(256), 0, as_stream(stream), src_kv_d, src_b, src_tmax, src_len_d, idx_d, dst_kv_d,
                       dst_tmax, b, d, src_hidden_d, src_last_x_d, dst_hidden_d, dst_last_x_d, dst_len_d);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_kv_attach_f32(int src_b, int src_tmax, const int32_t *src_len_d, const float *src_hidden_d, const float *src_last_x_d, const int32_t *idx_d,
                       int b, int dst_tmax, float *dst_hidden_d, float *dst_last_x_d, int32_t *dst_len_d, int32_t *pfx_n_d, int32_t *order_d, int d,
                       void *stream) {
    LMRL_REQUIRE(src_b > 0 && src_tmax > 0 && src_len_d && idx_d && b > 0 && dst_tmax > 0 && dst_len_d && pfx_n_d && d > 0 && d % 4 == 0,
                 "lmrl_kv_attach_f32: bad argument");
    LMRL_REQUIRE((!dst_hidden_d || src_hidden_d) && (!dst_last_x_d || src_last_x_d), "lmrl_kv_attach_f32: a destination row without its source");
    hipLaunchKernelGGL(kv_attach_f32_kernel, dim3(b + 1), dim3(1024), 0, as_stream(stream), src_b, src_tmax, src_len_d, idx_d, b, d, dst_tmax,
                       src_hidden_d, src_last_x_d, dst_hidden_d, dst_last_x_d, dst_len_d, pfx_n_d, order_d);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_kv_reorder_f32(const float *src_kv_d, const int32_t *src_len_d, const float *src_hidden_d, const float *src_last_x_d, const int32_t *parent_d,
                        const int32_t *from_d, float *dst_kv_d, int32_t *dst_len_d, float *dst_hidden_d, float *dst_last_x_d, int b, int tmax, int n_layer,
                        int d, const int32_t *go_d, void *stream) {
    LMRL_REQUIRE(src_kv_d && src_len_d && parent_d && dst_kv_d && dst_len_d && b > 0 && tmax > 0 && n_layer > 0 && d > 0 && d % 4 == 0,
                 "lmrl_kv_reorder_f32: bad argument");
    LMRL_REQUIRE(src_kv_d != dst_kv_d && src_len_d != dst_len_d, "lmrl_kv_reorder_f32: the copy is out of place (two caches of one shape)");
    LMRL_REQUIRE((!dst_hidden_d || src_hidden_d) && (!dst_last_x_d || src_last_x_d), "lmrl_kv_reorder_f32: a destination row without its source");
    hipLaunchKernelGGL(kv_reorder_f32_kernel, dim3(b, 2 * n_layer), dim3(256), 0, as_stream(stream), src_kv_d, src_len_d, parent_d, from_d, dst_kv_d, dst_len_d,
                       b, tmax, d, src_hidden_d, src_last_x_d, dst_hidden_d, dst_last_x_d, go_d);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

}  // extern "C"
