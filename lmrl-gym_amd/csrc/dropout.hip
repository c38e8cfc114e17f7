// dropout.hip — the elementwise dropout launches of the train step (embedding output, the two c_proj outputs of a block, and the attention
// probabilities of the materialized attention) and the host face of the mask stream.  The mask definition is csrc/dropout.h; the flash
// attention sweeps evaluate it inside their tile loops (csrc/flash_attn_train.hip).
//
// One kernel serves forward and backward: y = x * mask / (1 - p), in place or into another buffer (the backward writes dy * mask / (1 - p) into
// the buffer the producing GEMM's backward reads).  A thread owns the element pair (j, j + ceil(n / 2)): both keep bits come out of one
// Threefry block (dropout_keep_pair), so the launch costs ~55 integer ops per element against 8 bytes of traffic — at 256 CUs x 4 SIMDs x 16
// lanes that is about the time the HBM stream takes, and the grid is capped at 8 workgroups of 4 waves per CU (grid-stride beyond that).
#include "../../include/lmrl_amd.h"
#include "gemm_bf16.h"
#include "dropout.h"

namespace lmrl {

__global__ __launch_bounds__(256) void dropout_apply_kernel(const float *x, float *y, DropoutSite s) {      // y may be x
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < s.h; j += gridDim.x * 256u) {
        bool klo, khi;
        dropout_keep_pair(s, j, klo, khi);
        y[j] = klo ? x[j] * s.scale : 0.f;
        const uint32_t j2 = j + s.h;          // < 2^32: n < 2^32
        if (j2 < s.n) y[j2] = khi ? x[j2] * s.scale : 0.f;
    }
}

// x fp32 [rows][cols] -> bf16 [rows_dst][ldb] = x * mask / (1 - p) (zero beyond rows / cols): the dy operand of a c_proj backward in the
// bf16-matmul mode.  One workgroup per destination row, 8 consecutive columns per lane (one 16-byte store).
__global__ __launch_bounds__(256) void dropout_apply_bf16_kernel(const float *__restrict__ x, int rows, int cols, uint16_t *__restrict__ dst, long ldb,
                                                                 DropoutSite s) {
    const int r = blockIdx.x;
    uint16_t *q = dst + (size_t)r * ldb;
    const float *xr = x + (size_t)r * cols;
    for (int c0 = threadIdx.x * 8; c0 < ldb; c0 += 256 * 8) {
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool ok = r < rows && c0 + k < cols;
            float v = 0.f;
            if (ok) {
                const uint32_t i = (uint32_t)r * (uint32_t)cols + (uint32_t)(c0 + k);
                v = dropout_keep(s, i) ? xr[c0 + k] * s.scale : 0.f;
            }
            o[k] = v;
        }
        uint4 pk;
        pk.x = pack_bf16x2(o[0], o[1]); pk.y = pack_bf16x2(o[2], o[3]); pk.z = pack_bf16x2(o[4], o[5]); pk.w = pack_bf16x2(o[6], o[7]);
        *reinterpret_cast<uint4 *>(q + c0) = pk;
    }
}

static bool dropout_args_ok(uint64_t n, float p) { return n > 0 && n < (1ull << 32) && p > 0.f && p < 1.f; }

}  // namespace lmrl

using namespace lmrl;

extern "C" {

int lmrl_dropout_host_mask(uint32_t k0, uint32_t k1, uint32_t site, uint64_t n, float p, uint8_t *out) {
    LMRL_REQUIRE(out, "lmrl_dropout_host_mask: null pointer");
    LMRL_REQUIRE(n < (1ull << 32), "lmrl_dropout_host_mask: a dropout site holds fewer than 2^32 elements");
    LMRL_REQUIRE(n > 0 && p >= 0.f && p < 1.f, "lmrl_dropout_host_mask: bad argument");
    const DropoutSite s = dropout_site(k0, k1, site, (uint32_t)n, p);
    for (uint32_t i = 0; i < s.n; i++) out[i] = dropout_keep(s, i) ? 1 : 0;
    return LMRL_OK;
}

int lmrl_dropout_apply(const float *x_d, float *y_d, uint64_t n, uint32_t k0, uint32_t k1, uint32_t site, float p, void *stream) {
    LMRL_REQUIRE(x_d && y_d, "lmrl_dropout_apply: null pointer");
    LMRL_REQUIRE(n < (1ull << 32), "lmrl_dropout_apply: a dropout site holds fewer than 2^32 elements");
    LMRL_REQUIRE(dropout_args_ok(n, p), "lmrl_dropout_apply: bad argument (0 < p < 1)");
    const DropoutSite s = dropout_site(k0, k1, site, (uint32_t)n, p);
    const uint32_t blocks = (s.h + 255u) / 256u;
    hipLaunchKernelGGL(dropout_apply_kernel, dim3(blocks > 2048u ? 2048u : blocks), dim3(256), 0, as_stream(stream), x_d, y_d, s);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_dropout_apply_bf16(const float *x_d, int rows, int cols, void *dst_d, long ldb, int rows_dst, uint32_t k0, uint32_t k1, uint32_t site, float p,
                            void *stream) {
    LMRL_REQUIRE(x_d && dst_d && rows > 0 && cols > 0 && ldb >= cols && ldb % 8 == 0 && rows_dst >= rows, "lmrl_dropout_apply_bf16: bad argument");
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    LMRL_REQUIRE(n < (1ull << 32), "lmrl_dropout_apply_bf16: a dropout site holds fewer than 2^32 elements");
    LMRL_REQUIRE(dropout_args_ok(n, p), "lmrl_dropout_apply_bf16: bad argument (0 < p < 1)");
    const DropoutSite s = dropout_site(k0, k1, site, (uint32_t)n, p);
    hipLaunchKernelGGL(dropout_apply_bf16_kernel, dim3(rows_dst), dim3(256), 0, as_stream(stream), x_d, rows, cols, (uint16_t *)dst_d, ldb, s);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

}  // extern "C"
