// beam.hip — beam search on the device (num_beams of the policies' GenerationConfig): the per-step selection of HF-Flax `_beam_search`
// (transformers 4.26.1, restated in DESIGN.md "Beam search"; unverified against the library) as two launches on materialised logits.
//
//   lmrl_beam_row_topk   one workgroup per (item, beam) row: ONE pass over the row's logits with 16-byte loads — an online log-sum-exp over the
//                        true vocabulary and the row's 2K largest logits (ties: lower column).  The global top 2K of an item's K * V flattened
//                        log-probabilities lies in the union of its rows' top 2K.
//   lmrl_beam_select     one wave per item: top 2K of the K x 2K candidates, the next running beams, the merge into the finished pool, the
//                        gather of the token histories by parent, and the loop condition of the NEXT position.
//
// The -1e7 penalties of the rules (eos candidates among the running beams, unfinished candidates in the finished pool) are carried as a
// flag beside an fp32 value, never added into it: the kernel orders by (penalised, value) — the order of the float64 sums as long as the values
// stay far below 1e7 in magnitude — and fp32 scores keep their 24 bits.  In the finished pool `unflagged` IS `penalised` (a candidate that is
// flagged and penalised — a full pool under early stopping — never beats the K flagged entries of that pool), so fin_score holds the
// unpenalised value and an unflagged entry stands for fin_score - 1e7 (initially 0: the rules' -1e7).
//
// Stopping: the loop condition is global over the batch.  `ctl` is the caller's int32 [4][T + 1] (T = max_new_tokens), zeroed with ctl[0][0] = 1:
// row 0 = go[t] (position t runs), rows 1 / 2 = per-step accumulators (an item can still improve / an item's pool is not full), row 3 = arrival
// tickets.  Every kernel of position t returns at once when go[t] == 0; the item that arrives last at position t combines the accumulators
// into go[t + 1] and, when that is 0, clears next_cnt so that forwards enqueued past the stopping point append nothing.
#include "../../include/lmrl_amd.h"
#include "common.h"
#include <atomic>

namespace lmrl {

constexpr float kBeamNeg = -1.0e7f;

__device__ __forceinline__ uint32_t f32_orderable(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f32_from_orderable(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// larger value first, then the lower column
__device__ __forceinline__ unsigned long long topk_key(float v, int col) {
    return ((unsigned long long)f32_orderable(v + 0.0f) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)col);      // (-0 + 0 = +0: the zeros tie)
}

constexpr int kRowThreads = 256;

// lists: dynamic LDS, [nc][256] keys — thread t's list is column t (conflict-free); 0 = empty (below every finite logit's key)
__global__ __launch_bounds__(kRowThreads) void beam_row_topk_kernel(const float *__restrict__ logits, int ld, int V, int nc,
                                                                    const float *__restrict__ running_score, const uint8_t *__restrict__ active,
                                                                    const int32_t *__restrict__ go, float *__restrict__ cand_score,
                                                                    int32_t *__restrict__ cand_tok) {
    extern __shared__ unsigned long long lists[];
    __shared__ float red_m[kRowThreads / 64], red_s[kRowThreads / 64];
    __shared__ unsigned long long red_k[kRowThreads / 64];
    __shared__ unsigned long long win[32];
    if (go && *go == 0) return;
    const int row = blockIdx.x, tid = threadIdx.x;
    if (active && !active[row]) return;
    const float *x = logits + (size_t)row * ld;
    for (int j = 0; j < nc; j++) lists[j * kRowThreads + tid] = 0ull;
    unsigned long long kmin = 0ull;
    int jmin = 0;
    float m = -INFINITY, s = 0.f;
    for (int c = tid * 4; c < V; c += kRowThreads * 4) {
        const float4 q = *reinterpret_cast<const float4 *>(x + c);       // c + 3 < ld: ld is a multiple of 4 and c < V <= ld
        const float v4[4] = {q.x, q.y, q.z, q.w};
        float mx = m;
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (c + e < V) mx = fmaxf(mx, v4[e]);
        s *= expf(m - mx);                                               // (m = -inf, s = 0 on the first visit: 0 * exp(-inf) = 0)
        m = mx;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (c + e >= V) continue;
            s += expf(v4[e] - m);
            const unsigned long long key = topk_key(v4[e], c + e);
            if (key > kmin) {                                            // replaces this thread's smallest kept key
                lists[jmin * kRowThreads + tid] = key;
                kmin = lists[tid]; jmin = 0;
                for (int j = 1; j < nc; j++) {
                    const unsigned long long k2 = lists[j * kRowThreads + tid];
                    if (k2 < kmin) { kmin = k2; jmin = j; }
                }
            }
        }
    }
    // ---- log-sum-exp over the workgroup
    float wm = m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
    float ws = (m == -INFINITY) ? 0.f : s * expf(m - wm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ws += __shfl_xor(ws, o);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) { red_m[wave] = wm; red_s[wave] = ws; }
    __syncthreads();
    float gm = red_m[0];
    for (int w = 1; w < kRowThreads / 64; w++) gm = fmaxf(gm, red_m[w]);
    float gs = 0.f;
    for (int w = 0; w < kRowThreads / 64; w++) gs += (red_m[w] == -INFINITY) ? 0.f : red_s[w] * expf(red_m[w] - gm);
    const float lse = gm + logf(gs);
    // ---- the nc largest keys of the 256 lists, in descending order: nc rounds of a workgroup-wide maximum (keys are distinct: one per column)
    unsigned long long best = 0ull;
    int jbest = 0;
    for (int j = 0; j < nc; j++) {
        const unsigned long long k2 = lists[j * kRowThreads + tid];
        if (k2 > best) { best = k2; jbest = j; }
    }
    for (int r = 0; r < nc; r++) {
        unsigned long long wb = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(wb, o);
            wb = other > wb ? other : wb;
        }
        if (lane == 0) red_k[wave] = wb;
        __syncthreads();
        unsigned long long gb = red_k[0];
        for (int w = 1; w < kRowThreads / 64; w++) gb = red_k[w] > gb ? red_k[w] : gb;
        if (tid == 0) win[r] = gb;
        if (best == gb && gb != 0ull) {                                  // the one thread that holds it: drop it, find this list's next
            lists[jbest * kRowThreads + tid] = 0ull;
            best = 0ull; jbest = 0;
            for (int j = 0; j < nc; j++) {
                const unsigned long long k2 = lists[j * kRowThreads + tid];
                if (k2 > best) { best = k2; jbest = j; }
            }
        }
        __syncthreads();
    }
    if (tid < nc) {
        const unsigned long long k = win[tid];
        const float v = f32_from_orderable((uint32_t)(k >> 32));
        cand_score[(size_t)row * nc + tid] = (v - lse) + running_score[row];
        cand_tok[(size_t)row * nc + tid] = (int32_t)(0xffffffffu - (uint32_t)(k & 0xffffffffull));
    }
}

constexpr int kBeamMaxK = 16;                       // 2K <= 32 candidates per row
constexpr int kBeamMaxC = kBeamMaxK * 2 * kBeamMaxK; // K x 2K candidates of an item

struct BeamSelectArgs {
    const float *cand_score; const int32_t *cand_tok;                    // [B K][2K] of lmrl_beam_row_topk
    const float *run_score_in; float *run_score_out;                     // [B K]
    const int32_t *run_hist_in; int32_t *run_hist_out;                   // [B K][cap]
    const float *fin_score_in; float *fin_score_out;                     // [B K]
    const uint8_t *fin_flag_in; uint8_t *fin_flag_out;                   // [B K]
    const int32_t *fin_hist_in; int32_t *fin_hist_out;                   // [B K][cap]
    int32_t *parent, *next_tok, *next_cnt;                               // [B K]
    int32_t *ctl;                                                        // [4][T + 1]
    int B, K, V, cap, t, T, eos, pad, early_stopping, best_idx;
    float norm_div, best_div;
};

__global__ __launch_bounds__(64) void beam_select_kernel(BeamSelectArgs a) {
    __shared__ float s_score[kBeamMaxC];
    __shared__ uint32_t s_flat[kBeamMaxC];
    __shared__ float c_score[2 * kBeamMaxK];
    __shared__ int32_t c_beam[2 * kBeamMaxK], c_tok[2 * kBeamMaxK];
    __shared__ float m_val[3 * kBeamMaxK];
    __shared__ uint8_t m_pen[3 * kBeamMaxK];
    __shared__ int32_t f_src[kBeamMaxK];
    __shared__ float r_score[kBeamMaxK], f_score[kBeamMaxK];
    __shared__ uint8_t f_flag[kBeamMaxK];
    __shared__ int32_t r_parent[kBeamMaxK], r_tok[kBeamMaxK];
    const int T1 = a.T + 1;
    int32_t *go = a.ctl, *acc_improve = a.ctl + T1, *acc_open = a.ctl + 2 * T1, *ticket = a.ctl + 3 * T1;
    if (go[a.t] == 0) return;
    const int b = blockIdx.x, lane = threadIdx.x, K = a.K, NC = 2 * K, NCAND = K * NC, t = a.t;
    const size_t base = (size_t)b * K;
    // ---- 2. top 2K of the item's K x 2K candidates: rank = candidates that come before (larger score, then lower flat index beam * V + token)
    if (lane < NC) { c_score[lane] = -INFINITY; c_beam[lane] = 0; c_tok[lane] = 0; }      // (a rank no candidate takes — NaN scores — must not index)
    if (lane < K) { f_src[lane] = lane; f_score[lane] = 0.f; f_flag[lane] = 0; }
    for (int i = lane; i < NCAND; i += 64) {
        s_score[i] = a.cand_score[base * NC + i];
        s_flat[i] = (uint32_t)(i / NC) * (uint32_t)a.V + (uint32_t)min(max(a.cand_tok[base * NC + i], 0), a.V - 1);
    }
    __syncthreads();
    for (int i = lane; i < NCAND; i += 64) {
        const float sc = s_score[i];
        const uint32_t fl = s_flat[i];
        int rank = 0;
        for (int j = 0; j < NCAND; j++) {
            const float sj = s_score[j];
            rank += (sj > sc || (sj == sc && s_flat[j] < fl)) ? 1 : 0;
        }
        if (rank < NC) { c_score[rank] = sc; c_beam[rank] = i / NC; c_tok[rank] = (int32_t)(fl - (uint32_t)(i / NC) * (uint32_t)a.V); }
    }
    bool all_old = true;
    for (int k = 0; k < K; k++) all_old = all_old && a.fin_flag_in[base + k] != 0;
    const bool full = all_old && a.early_stopping;
    __syncthreads();
    // ---- 3 / 4. next running beams: the candidates in rank order, those that just finished behind all others (score - 1e7)
    const bool is_c = lane < NC;
    const bool fin = is_c && c_tok[lane] == a.eos;
    const unsigned long long m_fin = __ballot(fin), m_c = __ballot(is_c);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (is_c) {
        const int n_open = __popcll(m_c & ~m_fin);
        const int pos = fin ? n_open + __popcll(m_fin & below) : __popcll(m_c & ~m_fin & below);
        if (pos < K) {
            r_score[pos] = fin ? c_score[lane] + kBeamNeg : c_score[lane];
            r_parent[pos] = c_beam[lane];
            r_tok[pos] = c_tok[lane];
            a.parent[base + pos] = (int32_t)base + c_beam[lane];
            a.next_tok[base + pos] = c_tok[lane];
            a.next_cnt[base + pos] = 1;
            a.run_score_out[base + pos] = r_score[pos];
        }
        // ---- 5 - 7. the candidate's entry for the finished pool
        m_val[K + lane] = c_score[lane] / a.norm_div;
        m_pen[K + lane] = (!fin || full) ? 1 : 0;
    }
    if (lane < K) {
        m_val[lane] = a.fin_score_in[base + lane];
        m_pen[lane] = a.fin_flag_in[base + lane] ? 0 : 1;
    }
    __syncthreads();
    // ---- 8. merge [finished (K) | candidates (2K)], keep the top K: unpenalised first, then the larger value, then the lower merged index
    if (lane < K + NC) {
        const float v = m_val[lane];
        const int p = m_pen[lane];
        int rank = 0;
        for (int j = 0; j < K + NC; j++) {
            const int pj = m_pen[j];
            const float vj = m_val[j];
            rank += (pj < p || (pj == p && (vj > v || (vj == v && j < lane)))) ? 1 : 0;
        }
        if (rank < K) {
            f_src[rank] = lane;
            f_score[rank] = v;
            f_flag[rank] = lane < K ? (uint8_t)(a.fin_flag_in[base + lane] != 0) : (uint8_t)(c_tok[lane - K] == a.eos);
            a.fin_score_out[base + rank] = v;
            a.fin_flag_out[base + rank] = f_flag[rank];
        }
    }
    __syncthreads();
    // ---- token histories, gathered by parent (out of place: the buffers ping-pong)
    for (int k = 0; k < K; k++) {
        const int32_t *src = a.run_hist_in + (base + r_parent[k]) * a.cap;
        int32_t *dst = a.run_hist_out + (base + k) * a.cap;
        for (int p = lane; p < t; p += 64) dst[p] = src[p];
        if (lane == 0) dst[t] = r_tok[k];
        const int e = f_src[k];
        int32_t *fd = a.fin_hist_out + (base + k) * a.cap;
        if (e < K) {
            const int32_t *fs = a.fin_hist_in + (base + e) * a.cap;
            for (int p = lane; p < a.cap; p += 64) fd[p] = fs[p];
        } else {
            const int32_t *fs = a.run_hist_in + (base + c_beam[e - K]) * a.cap;
            const int32_t tk = c_tok[e - K];
            for (int p = lane; p < a.cap; p += 64) fd[p] = p < t ? fs[p] : (p == t ? tk : a.pad);
        }
    }
    // ---- the loop condition of position t + 1 (global over the batch).  Every lane publishes its own stores (next_cnt = 1 above among them) before
    // lane 0 takes the item's ticket: the last arriver's clearing of next_cnt is then ordered behind all of them.
    __threadfence();
    __syncthreads();
    if (lane == 0) {
        bool all_new = true;
        float worst = INFINITY;
        for (int k = 0; k < K; k++) {
            all_new = all_new && f_flag[k];
            worst = fminf(worst, f_flag[k] ? f_score[k] : f_score[k] + kBeamNeg);
        }
        const float best_running = r_score[a.best_idx] / a.best_div;
        // per beam: worst_finished = min(all pool scores) where the beam is flagged, -1e7 elsewhere; any beam below best_running keeps the item going
        bool improve = false;
        for (int k = 0; k < K; k++) improve = improve || ((f_flag[k] ? worst : kBeamNeg) < best_running);
        if (improve) atomicOr(&acc_improve[t], 1);
        if (!all_new) atomicOr(&acc_open[t], 1);
        __threadfence();
        if (atomicAdd(&ticket[t], 1) == a.B - 1) {
            __threadfence();
            const int imp = atomicOr(&acc_improve[t], 0), open = atomicOr(&acc_open[t], 0);
            const int g = (t + 1 < a.T) && imp && !(a.early_stopping && !open);
            go[t + 1] = g;
            if (!g)
                for (int i = 0; i < a.B * K; i++) a.next_cnt[i] = 0;
        }
    }
}

}  // namespace lmrl

using namespace lmrl;

extern "C" {

int lmrl_beam_row_topk(const float *logits_d, int ld, int rows, int vocab, int n_cand, const float *running_score_d, const uint8_t *active_d,
                       const int32_t *go_d, float *cand_score_d, int32_t *cand_tok_d, void *stream) {
    LMRL_REQUIRE(logits_d && running_score_d && cand_score_d && cand_tok_d && rows > 0, "lmrl_beam_row_topk: null pointer");
    LMRL_REQUIRE(vocab > 0 && vocab <= ld && ld % 4 == 0 && ((uintptr_t)logits_d & 15u) == 0, "lmrl_beam_row_topk: rows of 16-byte aligned float4s, vocab <= ld");
    LMRL_REQUIRE(n_cand > 0 && n_cand <= 32 && n_cand <= vocab, "lmrl_beam_row_topk: 1 <= n_cand <= min(32, vocab)");
    const size_t lds = (size_t)n_cand * kRowThreads * sizeof(unsigned long long);
    // 32 candidates: the lists alone fill 64 KB, and with the kernel's static LDS the launch passes the default limit — opt in to the largest list
    // size, once per device (a per-device function attribute; ranks / lanes may arrive from several host threads)
    static std::atomic<long> static_lds{-1};
    long st = static_lds.load(std::memory_order_acquire);
    if (st < 0) {
        hipFuncAttributes fa;
        LMRL_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&beam_row_topk_kernel)));
        st = (long)fa.sharedSizeBytes;
        static_lds.store(st, std::memory_order_release);
    }
    if (lds + (size_t)st > 65536) {
        static std::atomic<unsigned long long> attr_set{0ull};
        int dev_id = 0;
        LMRL_CHECK_HIP(hipGetDevice(&dev_id));
        const unsigned long long dev_bit = 1ull << (dev_id & 63);
        if (dev_id >= 64 || !(attr_set.load(std::memory_order_acquire) & dev_bit)) {
            LMRL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_row_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(32 * kRowThreads * sizeof(unsigned long long))));
            attr_set.fetch_or(dev_bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(beam_row_topk_kernel, dim3(rows), dim3(kRowThreads), lds, as_stream(stream),
                       logits_d, ld, vocab, n_cand, running_score_d, active_d, go_d, cand_score_d, cand_tok_d);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_beam_select(const lmrl_beam_state *in, const lmrl_beam_state *out, const float *cand_score_d, const int32_t *cand_tok_d, int32_t *parent_d,
                     int32_t *next_tok_d, int32_t *next_cnt_d, int32_t *ctl_d, int b, int num_beams, int vocab, int cap, int t, int max_new_tokens,
                     int eos_token, int pad_token, int early_stopping, int best_running_beam, float norm_div, float best_div, void *stream) {
    LMRL_REQUIRE(in && out && cand_score_d && cand_tok_d && parent_d && next_tok_d && next_cnt_d && ctl_d, "lmrl_beam_select: null pointer");
    LMRL_REQUIRE(in->run_score && in->run_hist && in->fin_score && in->fin_flag && in->fin_hist && out->run_score && out->run_hist && out->fin_score &&
                 out->fin_flag && out->fin_hist, "lmrl_beam_select: incomplete state");
    LMRL_REQUIRE(in->run_hist != out->run_hist && in->fin_hist != out->fin_hist && in->fin_score != out->fin_score && in->fin_flag != out->fin_flag &&
                 in->run_score != out->run_score, "lmrl_beam_select: the step is out of place (two states)");
    LMRL_REQUIRE(b > 0 && num_beams >= 1 && num_beams <= kBeamMaxK && vocab >= 2 * num_beams, "lmrl_beam_select: 1 <= num_beams <= 16, vocab >= 2 num_beams");
    LMRL_REQUIRE(max_new_tokens > 0 && t >= 0 && t < max_new_tokens && cap >= max_new_tokens, "lmrl_beam_select: 0 <= t < max_new_tokens <= cap");
    LMRL_REQUIRE(best_running_beam >= 0 && best_running_beam < num_beams && norm_div > 0.f && best_div > 0.f, "lmrl_beam_select: bad best_running_beam / divisor");
    BeamSelectArgs a{cand_score_d, cand_tok_d, in->run_score, out->run_score, in->run_hist, out->run_hist, in->fin_score, out->fin_score,
                     in->fin_flag, out->fin_flag, in->fin_hist, out->fin_hist, parent_d, next_tok_d, next_cnt_d, ctl_d,
                     b, num_beams, vocab, cap, t, max_new_tokens, eos_token, pad_token, early_stopping ? 1 : 0, best_running_beam, norm_div, best_div};
    hipLaunchKernelGGL(beam_select_kernel, dim3(b), dim3(64), 0, as_stream(stream), a);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

}  // extern "C"
