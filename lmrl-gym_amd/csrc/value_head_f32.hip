// value_head_f32.hip — the ILQL / MC value policy's LM head in exact fp32: three products and their combine in one launch.
//
//   pi = h . wte^T          q_i = qh_i . w2_i^T + b2_i          logits = fmaf(beta, q2 ? fminf(q1, q2) : q1, pi)
//
// (value_rl_base/gpt2/generation.py:100-119: pi_beta + beta * min(Q1, Q2), or pi_beta + beta * Q for the MC-returns policy, q2 == NULL.)
// Every product runs on v_mfma_f32_32x32x2_f32 with k in increasing order from a zero accumulator — the same chain, and so the same bits, as
// lmrl_sgemm of the same operands (a k-ordered fmaf chain, bias added after it).  A workgroup owns a 128 x 128 output tile and runs Q1, then
// Q2 (folded in with fminf), then pi_beta in sequence: two 64-register accumulator sets per lane are live at once.  The combined logits are
// written once; no Q logits reach HBM, there is no split-K, no workspace and no device state (deterministic, capturable).
// The combine is one fmaf (one rounding); the bf16 sampler's `v += beta * qmin` is built with -ffp-contract=off and rounds the product first.
#include "../../include/lmrl_amd.h"
#include "common.h"

namespace lmrl {

typedef __attribute__((ext_vector_type(16))) float vh_f32x16;
typedef __attribute__((ext_vector_type(4))) float vh_f32x4;

constexpr int VH_BM = 128, VH_BN = 128, VH_BK = 16, VH_LD = 132;   // LDS row stride 132 % 32 = 4: k-major stores spread over the banks

// One K-step of a [128 rows][16 k] tile of a k-contiguous [rows][ld] operand: thread t loads row t >> 1, k (t & 1) * 8 .. + 7 as two float4
// (rows >= nrows read as zero: the h / qh operands' last row block).  K is a multiple of 64 and rows are 16-byte aligned (checked at the entry).
__device__ __forceinline__ void vh_load(const float *__restrict__ X, int ld, int row0, int nrows, int k0, int t, float (&r)[8]) {
    const int row = row0 + (t >> 1);
    if (row < nrows) {
        const float *p = X + (size_t)row * ld + k0 + (t & 1) * 8;
        const vh_f32x4 v0 = *reinterpret_cast<const vh_f32x4 *>(p), v1 = *reinterpret_cast<const vh_f32x4 *>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; i++) { r[i] = v0[i]; r[4 + i] = v1[i]; }
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) r[i] = 0.f;
    }
}
__device__ __forceinline__ void vh_store(float *__restrict__ S, int t, const float (&r)[8]) {
    const int row = t >> 1, k = (t & 1) * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) S[(k + i) * VH_LD + row] = r[i];
}

// acc[a][b] = A[m0 + wm 64 + a 32 ..][0, K) . B[n0 + wn 64 + b 32 ..][0, K)^T, k in order — the loop of sgemm_f32_128_kernel (loads two K-steps
// ahead of their use).  Ends on a barrier: the next product may overwrite both LDS buffers.
__device__ __forceinline__ void vh_product(const float *__restrict__ A, int nrows_a, const float *__restrict__ B, int K, int m0, int n0,
                                           float (*sA)[VH_BK * VH_LD], float (*sB)[VH_BK * VH_LD], vh_f32x16 (&acc)[2][2]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[a][b][i] = 0.f;
    float rca[8], rcb[8], rna[8], rnb[8];
    const int nk = K / VH_BK;
    vh_load(A, K, m0, nrows_a, 0, t, rca);
    vh_load(B, K, n0, 0x7fffffff, 0, t, rcb);
    vh_store(sA[0], t, rca);
    vh_store(sB[0], t, rcb);
    if (nk > 1) { vh_load(A, K, m0, nrows_a, VH_BK, t, rca); vh_load(B, K, n0, 0x7fffffff, VH_BK, t, rcb); }
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int buf = kt & 1;
        if (kt + 2 < nk) { vh_load(A, K, m0, nrows_a, (kt + 2) * VH_BK, t, rna); vh_load(B, K, n0, 0x7fffffff, (kt + 2) * VH_BK, t, rnb); }
        const float *pa = sA[buf] + (lane >> 5) * VH_LD + wm * 64 + (lane & 31);
        const float *pb = sB[buf] + (lane >> 5) * VH_LD + wn * 64 + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < VH_BK; kk += 2) {
            const float a0 = pa[kk * VH_LD], a1 = pa[kk * VH_LD + 32];
            const float b0 = pb[kk * VH_LD], b1 = pb[kk * VH_LD + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (kt + 1 < nk) { vh_store(sA[buf ^ 1], t, rca); vh_store(sB[buf ^ 1], t, rcb); }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; i++) { rca[i] = rna[i]; rcb[i] = rnb[i]; }
    }
}

// acc += bias[col] per output column (sgemm's epilogue: alpha = 1 times the chain, plus the bias)
__device__ __forceinline__ void vh_add_bias(vh_f32x16 (&acc)[2][2], const float *__restrict__ bias, int n0) {
    const int lane = threadIdx.x & 63, wn = (threadIdx.x >> 6) & 1;
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const float bv = bias[n0 + wn * 64 + b * 32 + (lane & 31)];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = acc[a][b][r] + bv;
    }
}

struct ValueHeadArgs {
    const float *h, *wte, *qh1, *w2_1, *b2_1, *qh2, *w2_2, *b2_2;
    float beta;
    int m, d, tiles_m, tiles_n;
    float *logits;
    int ld;
};

__global__ __launch_bounds__(256) void value_head_f32_kernel(ValueHeadArgs g) {
    __shared__ float sA[2][VH_BK * VH_LD];
    __shared__ float sB[2][VH_BK * VH_LD];
    // tile order: with a grid that is a multiple of the 8 XCDs (workgroups go round-robin over them), XCD x takes a contiguous run of tiles,
    // row blocks fastest — the row blocks of one column tile share its three [128][d] weight slices in that XCD's L2
    const int nwg = g.tiles_m * g.tiles_n;
    int v = blockIdx.x;
    if (nwg % 8 == 0) v = (v & 7) * (nwg >> 3) + (v >> 3);
    const int m0 = (v % g.tiles_m) * VH_BM, n0 = (v / g.tiles_m) * VH_BN;

    vh_f32x16 q[2][2], p[2][2];
    vh_product(g.qh1, g.m, g.w2_1, g.d, m0, n0, sA, sB, q);
    vh_add_bias(q, g.b2_1, n0);
    if (g.qh2) {
        vh_product(g.qh2, g.m, g.w2_2, g.d, m0, n0, sA, sB, p);
        vh_add_bias(p, g.b2_2, n0);
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) q[a][b][r] = fminf(q[a][b][r], p[a][b][r]);
    }
    vh_product(g.h, g.m, g.wte, g.d, m0, n0, sA, sB, p);

    // C/D layout of 32x32: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const int col = n0 + wn * 64 + b * 32 + (lane & 31);
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = m0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < g.m) g.logits[(size_t)row * g.ld + col] = __builtin_fmaf(g.beta, q[a][b][r], p[a][b][r]);
            }
    }
}

}  // namespace lmrl

using namespace lmrl;

static bool vh_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int lmrl_value_head_logits_f32(const float *h_d, const float *wte_d, const float *qh1_d, const float *w2_1_d, const float *b2_1_d,
                               const float *qh2_d, const float *w2_2_d, const float *b2_2_d, float beta, int m, int d, int vocab_padded,
                               float *logits_d, int ld, void *stream) {
    LMRL_REQUIRE(h_d && wte_d && qh1_d && w2_1_d && b2_1_d && logits_d, "lmrl_value_head_logits_f32: null pointer");
    LMRL_REQUIRE((qh2_d == nullptr) == (w2_2_d == nullptr) && (qh2_d == nullptr) == (b2_2_d == nullptr),
                 "lmrl_value_head_logits_f32: qh2, w2_2 and b2_2 are all given (ILQL) or all NULL (MC)");
    LMRL_REQUIRE(m > 0 && d > 0 && d % 64 == 0 && vocab_padded > 0 && vocab_padded % VH_BN == 0 && ld >= vocab_padded,
                 "lmrl_value_head_logits_f32: bad shape (m > 0, d % 64 == 0, vocab_padded % 128 == 0, ld >= vocab_padded)");
    LMRL_REQUIRE(vh_aligned(h_d) && vh_aligned(wte_d) && vh_aligned(qh1_d) && vh_aligned(w2_1_d) && (!qh2_d || (vh_aligned(qh2_d) && vh_aligned(w2_2_d))),
                 "lmrl_value_head_logits_f32: h / wte / qh / w2 must be 16-byte aligned");
    const long tiles = (long)ceil_div(m, VH_BM) * (vocab_padded / VH_BN);
    LMRL_REQUIRE(tiles < 0x7fffffffL, "lmrl_value_head_logits_f32: grid too large");
    ValueHeadArgs g{h_d, wte_d, qh1_d, w2_1_d, b2_1_d, qh2_d, w2_2_d, b2_2_d, beta, m, d, ceil_div(m, VH_BM), vocab_padded / VH_BN, logits_d, ld};
    hipLaunchKernelGGL(value_head_f32_kernel, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), g);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}
