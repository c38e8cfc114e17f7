// attn_rope_f32.hip — the two kernels GPT-J's attention adds to the fp32 rollout mode (GPTJEngineF32): the rotary position embedding applied
// in place to q and k, and cached causal attention at head dim 64 / 128 / 256.
//
// Rotary embedding (HF PyTorch GPT-J, `apply_rotary_pos_emb` + `rotate_every_two`): the first `rotary_dim` dims of every q and k head are
// rotated pairwise, interleaved — pair i = dims (2i, 2i + 1):
//     y[2i] = x[2i] cos - x[2i+1] sin        y[2i+1] = x[2i+1] cos + x[2i] sin
// with sin / cos of angle pos * 10000^(-2i / rotary_dim) read from an fp32 table [n_pos][rotary_dim] = [sin(0 .. rd/2) | cos(0 .. rd/2)] that the
// host builds exactly as HF's `create_sinusoidal_positions` does: the kernel computes no transcendental function.  Two rounded products and one
// rounded add per output (-ffp-contract=off), the order of HF's fp32 expression.  v, the dims >= rotary_dim and rows with pos < 0 are not touched.
//
// Attention: same cache layout and arguments as csrc/attn_cached_f32.hip (kcache / vcache fp32 [B][tmax][H * Dh], qkv fp32 [B * C][3 * H * Dh],
// ragged len / cnt, the C new rows appended to the cache, keys of the chunk itself read from `qkv`), with the head dim a template parameter.
// One wave per (env, head, query).  A K / V row of Dh floats is Dh / 4 float4 columns, held by LPR = Dh / 4 lanes (16 / 32 / 64); a wave
// instruction therefore covers G = 64 / LPR key positions (4 / 2 / 1).  Keys are walked in tiles of kKeyTile = 8 positions: the tile's K and V
// float4s are all requested before any arithmetic (8 / G loads of each per lane), scores are 4 fmaf per lane summed over the LPR lanes of a row,
// the online softmax (fp32, expf) rescales once per tile, and the G position slots are merged at the end.  fp32 throughout.
#include "../../include/lmrl_amd.h"
#include "common.h"

#include <vector>

namespace lmrl {

constexpr int kKeyTile = 8;      // key positions per tile of attn_hd_f32_kernel (lmrl_attn_hd_key_tile)

// one thread per (row, q | k, head, pair): an 8-byte vector load and store
__global__ __launch_bounds__(256) void rope_gptj_f32_kernel(float *__restrict__ qkv, const int32_t *__restrict__ pos, const float *__restrict__ sincos,
                                                            long total, int H, int Dh, int rd, int n_pos) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int half = rd >> 1;
    const int pair = (int)(i % half);
    long r = i / half;
    const int h = (int)(r % H); r /= H;
    const int which = (int)(r & 1);                                    // 0: q, 1: k
    const long row = r >> 1;
    const int p = pos[row];
    if (p < 0 || p >= n_pos) return;                                   // dead slot / outside the table: the row passes through, nothing is read
    const float sn = sincos[(size_t)p * rd + pair], cs = sincos[(size_t)p * rd + half + pair];
    float2 *at = reinterpret_cast<float2 *>(qkv + (size_t)row * 3 * H * Dh + (size_t)which * H * Dh + (size_t)h * Dh + 2 * pair);
    const float2 x = *at;
    *at = float2{x.x * cs - x.y * sn, x.y * cs + x.x * sn};
}

template <int DH>
__global__ __launch_bounds__(256) void attn_hd_f32_kernel(const float *__restrict__ qkv, float *__restrict__ kcache, float *__restrict__ vcache,
                                                            const int32_t *__restrict__ len, const int32_t *__restrict__ cnt,
                                                            float *__restrict__ out, int B, int C, int H, int tmax, float scale) {
    constexpr int LPR = DH / 4;              // lanes per K / V row
    constexpr int G = 64 / LPR;              // key positions per wave instruction
    constexpr int U = kKeyTile / G;          // loads of K (and of V) per lane and tile
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);          // wave id = ((b * C) + j) * H + h
    if (w >= (long)B * C * H) return;
    const int h = (int)(w % H);
    const int j = (int)((w / H) % C);
    const int b = (int)(w / ((long)H * C));
    if (j >= cnt[b]) return;                                           // padding slot (wave-uniform): `out` untouched
    const int L = len[b];
    if (L < 0 || L + j >= tmax) return;                                // no room in the cache (the engine refuses such a forward on the host)
    const int d = H * DH;
    const int g = lane / LPR, c = lane % LPR;
    const float *rows = qkv + (size_t)b * C * 3 * d + h * DH + c * 4; // this env's chunk rows, at this lane's float4 column of head h
    const float4 q4 = *reinterpret_cast<const float4 *>(rows + (size_t)j * 3 * d);
    float *kc = kcache + (size_t)b * tmax * d + h * DH + c * 4;
    float *vc = vcache + (size_t)b * tmax * d + h * DH + c * 4;
    if (g == 0) {                                                      // append this token's K / V row (read back below only from `qkv`)
        *reinterpret_cast<float4 *>(kc + (size_t)(L + j) * d) = *reinterpret_cast<const float4 *>(rows + (size_t)j * 3 * d + d);
        *reinterpret_cast<float4 *>(vc + (size_t)(L + j) * d) = *reinterpret_cast<const float4 *>(rows + (size_t)j * 3 * d + 2 * d);
    }
    const int n = L + j + 1;                                           // visible keys: cached [0, L) + this chunk's tokens [0, j]
    float m = -1e30f, l = 0.f;
    float4 o = {0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < n; t0 += kKeyTile) {                         // wave-uniform trip count
        float4 kr[U], vr[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (t0 + u * G < n) {                                      // wave-uniform
                const int t = min(t0 + u * G + g, n - 1);
                const float *kp = t < L ? kc + (size_t)t * d : rows + (size_t)(t - L) * 3 * d + d;
                const float *vp = t < L ? vc + (size_t)t * d : rows + (size_t)(t - L) * 3 * d + 2 * d;
                kr[u] = *reinterpret_cast<const float4 *>(kp);
                vr[u] = *reinterpret_cast<const float4 *>(vp);
            }
        float sc[U];
        float mb = m;
#pragma unroll
        for (int u = 0; u < U; u++) {
            sc[u] = -1e30f;
            if (t0 + u * G < n) {
                float s = fmaf(q4.x, kr[u].x, fmaf(q4.y, kr[u].y, fmaf(q4.z, kr[u].z, q4.w * kr[u].w)));
#pragma unroll
                for (int x = 1; x < LPR; x <<= 1) s += __shfl_xor(s, x);
                s *= scale;
                if (t0 + u * G + g < n) { sc[u] = s; mb = fmaxf(mb, s); }
            }
        }
        const float alpha = expf(m - mb);
        l *= alpha; o.x *= alpha; o.y *= alpha; o.z *= alpha; o.w *= alpha;
#pragma unroll
        for (int u = 0; u < U; u++)
            if (t0 + u * G < n) {
                const float pr = (t0 + u * G + g < n) ? expf(sc[u] - mb) : 0.f;
                l += pr;
                o.x = fmaf(pr, vr[u].x, o.x); o.y = fmaf(pr, vr[u].y, o.y); o.z = fmaf(pr, vr[u].z, o.z); o.w = fmaf(pr, vr[u].w, o.w);
            }
        m = mb;
    }
    // merge the G position slots (a slot that saw no key has m = -1e30, l = 0: weight exp(-1e30 - mm) = 0; slot 0 always holds position 0)
    float mm = m;
#pragma unroll
    for (int x = LPR; x < 64; x <<= 1) mm = fmaxf(mm, __shfl_xor(mm, x));
    const float wgt = expf(m - mm);
    float lt = l * wgt;
    float4 r = {o.x * wgt, o.y * wgt, o.z * wgt, o.w * wgt};
#pragma unroll
    for (int x = LPR; x < 64; x <<= 1) {
        lt += __shfl_xor(lt, x);
        r.x += __shfl_xor(r.x, x); r.y += __shfl_xor(r.y, x); r.z += __shfl_xor(r.z, x); r.w += __shfl_xor(r.w, x);
    }
    if (g == 0) {
        const float inv = 1.f / lt;
        *reinterpret_cast<float4 *>(out + ((size_t)b * C + j) * d + h * DH + c * 4) = float4{r.x * inv, r.y * inv, r.z * inv, r.w * inv};
    }
}

static int rope_check_args(const float *qkv_d, const int32_t *pos_d, const float *sincos_d, int rows, int n_head, int head_dim, int rotary_dim, int n_pos,
                           const char *who) {
    if (!(qkv_d && pos_d && sincos_d && rows > 0 && n_head > 0 && n_pos > 0)) { set_error("%s: bad argument", who); return LMRL_ERR_ARG; }
    if (!(head_dim > 0 && head_dim % 2 == 0 && rotary_dim > 0 && rotary_dim % 2 == 0 && rotary_dim <= head_dim)) {
        set_error("%s: rotary_dim = %d must be even and within head_dim = %d (even)", who, rotary_dim, head_dim);
        return LMRL_ERR_ARG;
    }
    return LMRL_OK;
}

}  // namespace lmrl

using namespace lmrl;

extern "C" {

int lmrl_attn_hd_key_tile(void) { return kKeyTile; }

int lmrl_rope_gptj_f32_async(float *qkv_d, const int32_t *pos_d, const float *sincos_d, int rows, int n_head, int head_dim, int rotary_dim, int n_pos,
                             void *stream) {
    const int rc = rope_check_args(qkv_d, pos_d, sincos_d, rows, n_head, head_dim, rotary_dim, n_pos, "lmrl_rope_gptj_f32_async");
    if (rc != LMRL_OK) return rc;
    const long total = (long)rows * 2 * n_head * (rotary_dim / 2);
    hipLaunchKernelGGL(rope_gptj_f32_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), qkv_d, pos_d, sincos_d, total, n_head, head_dim,
                       rotary_dim, n_pos);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_rope_gptj_f32(float *qkv_d, const int32_t *pos_d, const float *sincos_d, int rows, int n_head, int head_dim, int rotary_dim, int n_pos,
                       void *stream) {
    const int rc = rope_check_args(qkv_d, pos_d, sincos_d, rows, n_head, head_dim, rotary_dim, n_pos, "lmrl_rope_gptj_f32");
    if (rc != LMRL_OK) return rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    LMRL_CHECK_HIP(hipStreamIsCapturing(as_stream(stream), &cap));
    LMRL_REQUIRE(cap == hipStreamCaptureStatusNone,
                 "lmrl_rope_gptj_f32 reads the positions back and cannot run in a stream capture (lmrl_rope_gptj_f32_async does not)");
    std::vector<int32_t> pos((size_t)rows);
    LMRL_CHECK_HIP(hipMemcpyAsync(pos.data(), pos_d, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, as_stream(stream)));
    LMRL_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    for (int r = 0; r < rows; r++)
        if (pos[(size_t)r] >= n_pos) {
            set_error("lmrl_rope_gptj_f32: row %d has position %d, the sin / cos table holds %d", r, pos[(size_t)r], n_pos);
            return LMRL_ERR_ARG;
        }
    return lmrl_rope_gptj_f32_async(qkv_d, pos_d, sincos_d, rows, n_head, head_dim, rotary_dim, n_pos, stream);
}

int lmrl_attn_cached_hd_f32(const float *qkv_d, float *kcache_d, float *vcache_d, const int32_t *len_d, const int32_t *cnt_d, float *out_d, int b, int c,
                              int n_head, int head_dim, int tmax, void *stream) {
    LMRL_REQUIRE(qkv_d && kcache_d && vcache_d && len_d && cnt_d && out_d && b > 0 && c > 0 && n_head > 0 && tmax > 0,
                 "lmrl_attn_cached_hd_f32: bad argument");
    LMRL_REQUIRE(head_dim == 64 || head_dim == 128 || head_dim == 256, "lmrl_attn_cached_hd_f32: head_dim must be 64, 128 or 256");
    const dim3 grid(ceil_div((long)b * c * n_head, 4)), block(256);
    hipStream_t s = as_stream(stream);
    // 1 / sqrt(head_dim): a power of two at 64 and 256, the correctly rounded float at 128
    if (head_dim == 64)
        hipLaunchKernelGGL(attn_hd_f32_kernel<64>, grid, block, 0, s, qkv_d, kcache_d, vcache_d, len_d, cnt_d, out_d, b, c, n_head, tmax, 0.125f);
    else if (head_dim == 128)
        hipLaunchKernelGGL(attn_hd_f32_kernel<128>, grid, block, 0, s, qkv_d, kcache_d, vcache_d, len_d, cnt_d, out_d, b, c, n_head, tmax,
                           0.08838834764831845f);
    else
        hipLaunchKernelGGL(attn_hd_f32_kernel<256>, grid, block, 0, s, qkv_d, kcache_d, vcache_d, len_d, cnt_d, out_d, b, c, n_head, tmax, 0.0625f);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

}  // extern "C"
