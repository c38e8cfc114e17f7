// offline_data.hip — rollout records -> the blocked ILQL / MC / BC datasets, without leaving the device (gfx950).
//
// Reference: the offline trainers' data path.  wordle/misc/data_gen.py:53-62 writes jsonl items; train_ilql_gpt2.py:123-152 reads them back,
// tokenises every episode (TokenTrajectoryChain.from_text_trajectory_chain, LLM_RL/environment.py:349-420) and blocks
// ILQLData.from_token_trajectory_chain / MCData.from_token_trajectory_chain (ilql/data.py:18-79, mc_returns/data.py:21-74) or the
// (ids, training mask) pairs of MaskIterableDataset (train_bc_gpt2.py) with JaxSeq's block_sequences.  Here the records a device loop left in
// HBM go straight to those blocked arrays:
//
//   lmrl_wordle_tok_scripted_records   guess / obs / reward / flags / n_turns of lmrl_wordle_policy_episodes -> lmrl_ppo_records rows
//                                      (the per-episode rule is offline_data_core.h; lmrl_wordle_host_scripted_record is its host face)
//   lmrl_offline_block                 any lmrl_ppo_records (+ a list of kept rows) -> input_ids, should_take_action, rewards, returns,
//                                      training mask, dones, lengths and, for multi-trajectory chains, next_token_ids / next_dones
//   lmrl_record_returns                undiscounted reward sum per chain (the %BC filtering score)
//
// Mapping, as in ppo_data.hip: one 64-lane wave per trajectory, lanes over token slots, so every wave instruction reads / writes one
// contiguous run of a row.  All of it is HBM-bound streaming of a few hundred bytes per episode.
#include "../../include/lmrl_amd.h"
#include "common.h"
#include "offline_data_core.h"

namespace lmrl {

__device__ __forceinline__ int clamp_len(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

__global__ __launch_bounds__(256) void scripted_records_kernel(lmrl_wordle_tokens t, const uint32_t *__restrict__ guess, const uint32_t *__restrict__ obs,
                                                               const float *__restrict__ reward, const uint8_t *__restrict__ flags,
                                                               const int32_t *__restrict__ n_turns, int stride, int n, int cap,
                                                               int32_t *__restrict__ tokens, uint8_t *__restrict__ is_action, float *__restrict__ rew,
                                                               int32_t *__restrict__ n_tok, uint8_t *__restrict__ done, int32_t *__restrict__ err) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + wave;
    if (e >= n) return;
    WordleEpisode ep;
    ep.n_turns = clamp_len(n_turns[e], kWordleTries);
    bool bad = false;
    for (int k = 0; k < kWordleTries; k++) {              // the same 4-byte words in every lane: one broadcast load each
        const bool played = k < ep.n_turns;
        ep.guess[k] = played ? guess[(size_t)k * stride + e] : 0u;
        ep.obs[k] = played ? obs[(size_t)k * stride + e] : 0u;
        ep.reward[k] = played ? reward[(size_t)k * stride + e] : 0.f;
        bad = bad || (played && (flags[(size_t)k * stride + e] & 8u));      // the policy had no word left: not an episode of the reference
    }
    const int nt = wordle_episode_ntok(t, ep);
    for (int base = 0; base < cap; base += 64) {
        const int s = base + lane;
        if (s >= cap) break;
        int32_t tok = t.pad; uint8_t ia = 0; float rw = 0.f;
        wordle_episode_slot(t, ep, s, tok, ia, rw);
        const size_t o = (size_t)e * cap + s;
        tokens[o] = tok; is_action[o] = ia; rew[o] = rw;
    }
    if (lane == 0) {
        n_tok[e] = nt < cap ? nt : cap;
        done[e] = (ep.n_turns > 0 && (flags[(size_t)(ep.n_turns - 1) * stride + e] & 1u)) ? 1 : 0;
        if (err && (bad || nt > cap)) atomicAdd(err, 1);
    }
}

struct Records {                  // lmrl_ppo_records, device pointers
    const int32_t *tokens; const uint8_t *is_action; const float *reward; const int32_t *n_tok; const uint8_t *done;
    const int32_t *chain; const uint8_t *last;
    int n, cap, n_chains;
};

// block_sequences(Padding.RIGHT) of one sequence of `len` elements to width w: element t of the row is source element off + t (t < min(len, w)),
// off = len - w under Truncation.LEFT when len > w, else 0
__device__ __forceinline__ void block_span(int len, int w, bool left, int &kept, int &off) {
    kept = len < w ? len : w;
    off = (left && len > w) ? len - w : 0;
}

__global__ __launch_bounds__(256) void offline_block_kernel(Records r, const int32_t *__restrict__ keep, int m, int T, int pad, int left,
                                                            const float *__restrict__ returns, int ret_pitch, lmrl_offline_blocks o) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + wave;
    if (j >= m) return;
    int k = keep ? keep[j] : j;
    const bool row_ok = k >= 0 && k < r.n;              // a kept-row index outside the records gives an all-padding row
    k = row_ok ? k : 0;
    const int nn = row_ok ? clamp_len(r.n_tok[k], r.cap) : 0;
    const int32_t *trow = r.tokens + (size_t)k * r.cap;
    const uint8_t *arow = r.is_action + (size_t)k * r.cap;
    const float *wrow = r.reward + (size_t)k * r.cap;
    int len, off;
    block_span(nn, T, left != 0, len, off);
    for (int t = lane; t < T; t += 64) {
        const bool in = t < len;
        o.input_ids[(size_t)j * T + t] = in ? trow[off + t] : pad;
        if (o.training_mask) o.training_mask[(size_t)j * T + t] = (in && arow[off + t] != 0) ? 1.f : 0.f;
    }
    // the [T - 1] arrays are sequences of nn - 1 elements (x[1:]) blocked with max_length - 1 on their own (ILQLData.block / MCData.block)
    const int T1 = T - 1;
    int len1, off1;
    block_span(nn > 0 ? nn - 1 : 0, T1, left != 0, len1, off1);
    for (int t = lane; t < T1; t += 64) {
        const bool in = t < len1;
        const size_t q = (size_t)j * T1 + t;
        if (o.should_take_action) o.should_take_action[q] = (in && arow[1 + off1 + t] != 0) ? 1 : 0;
        if (o.rewards) o.rewards[q] = in ? wrow[1 + off1 + t] : 0.f;
        if (o.returns) o.returns[q] = (in && returns && off1 + t < ret_pitch) ? returns[(size_t)k * ret_pitch + off1 + t] : 0.f;
    }
    const bool is_last = r.last ? r.last[k] != 0 : true;
    const int c = r.chain ? r.chain[k] : k;
    const bool chain_done = c >= 0 && c < r.n_chains && r.done[c] != 0;
    if (lane == 0) {
        if (o.dones) o.dones[j] = (row_ok && is_last && chain_done) ? 1 : 0;      // an earlier trajectory of a chain is never done
        o.lengths[j] = len;
    }
    if (!o.next_token_ids) return;
    // ILQLData.from_token_trajectory_chain (ilql/data.py:62-71): the next trajectory's tokens up to (excluding) its first action at index >= 1,
    // next_done = False; without such an action the whole trajectory and its own done.  The chain's last trajectory has no successor (None in
    // the reference, which cannot be blocked): an all-padding row with next_done = 1, i.e. a zero bootstrap.
    const bool has = row_ok && r.chain && !is_last && k + 1 < r.n && r.chain[k + 1] == r.chain[k];
    int nlen = 0;
    bool ndone = true;
    const int q = k + 1;
    if (has) {
        const int nq = clamp_len(r.n_tok[q], r.cap);
        const uint8_t *qa = r.is_action + (size_t)q * r.cap;
        int first = -1;
        for (int base = 1; base < nq && first < 0; base += 64) {
            const int t = base + lane;
            const unsigned long long bal = __ballot(t < nq && qa[t] != 0);
            if (bal) first = base + (__ffsll((long long)bal) - 1);
        }
        nlen = first >= 0 ? first : nq;
        ndone = first >= 0 ? false : ((r.last ? r.last[q] != 0 : true) && chain_done);
    }
    int nkept, noff;
    block_span(nlen, T, left != 0, nkept, noff);
    const int32_t *qrow = r.tokens + (size_t)(has ? q : k) * r.cap;
    for (int t = lane; t < T; t += 64) o.next_token_ids[(size_t)j * T + t] = t < nkept ? qrow[noff + t] : pad;
    if (lane == 0) {
        if (o.next_dones) o.next_dones[j] = ndone ? 1 : 0;
        if (o.next_lengths) o.next_lengths[j] = nkept;
    }
}

// sum of every reward of a chain, in trajectory then token order per lane, lanes added in a fixed tree, in double; the wave of a chain's FIRST
// trajectory walks the chain (its trajectories are consecutive rows)
__global__ __launch_bounds__(256) void record_returns_kernel(Records r, float *__restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + wave;
    if (k >= r.n) return;
    if (r.chain && k > 0 && r.chain[k] == r.chain[k - 1]) return;
    const int c = r.chain ? r.chain[k] : k;
    double s = 0.0;
    for (int kk = k; kk < r.n && (r.chain ? r.chain[kk] == c : kk == k); kk++) {
        const int nn = clamp_len(r.n_tok[kk], r.cap);
        for (int t = lane; t < nn; t += 64) s += (double)r.reward[(size_t)kk * r.cap + t];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    if (lane == 0 && c >= 0 && c < r.n_chains) out[c] = (float)s;
}

static bool records_ok(const lmrl_ppo_records *r) {
    return r && r->tokens && r->is_action && r->reward && r->n_tok && r->done && r->n > 0 && r->cap > 0 && r->n_chains > 0 && r->n_chains <= r->n &&
           ((r->chain != nullptr) == (r->last != nullptr)) && (r->chain || r->n_chains == r->n);
}

static Records records_of(const lmrl_ppo_records *r) { return Records{r->tokens, r->is_action, r->reward, r->n_tok, r->done, r->chain, r->last, r->n, r->cap, r->n_chains}; }

}  // namespace lmrl

using namespace lmrl;

extern "C" {

int lmrl_wordle_tok_scripted_records(const lmrl_wordle_tokens *tokens, const uint32_t *guess_d, const uint32_t *obs_d, const float *reward_d,
                                     const uint8_t *flags_d, const int32_t *n_turns_d, int stride, int n, int cap, int32_t *tokens_d,
                                     uint8_t *is_action_d, float *rec_reward_d, int32_t *n_tok_d, uint8_t *done_d, int32_t *err_d, void *stream) {
    LMRL_REQUIRE(tokens && guess_d && obs_d && reward_d && flags_d && n_turns_d && tokens_d && is_action_d && rec_reward_d && n_tok_d && done_d,
                 "lmrl_wordle_tok_scripted_records: bad argument");
    LMRL_REQUIRE(n > 0 && stride >= n && cap > 0 && tokens->n_header >= 0 && tokens->n_header <= 8, "lmrl_wordle_tok_scripted_records: bad shape");
    hipStream_t s = as_stream(stream);
    if (err_d) LMRL_CHECK_HIP(hipMemsetAsync(err_d, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(scripted_records_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, s, *tokens, guess_d, obs_d, reward_d, flags_d, n_turns_d, stride, n, cap,
                       tokens_d, is_action_d, rec_reward_d, n_tok_d, done_d, err_d);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_wordle_host_scripted_record(const lmrl_wordle_tokens *tokens, const uint32_t *guess6, const uint32_t *obs6, const float *reward6,
                                     const uint8_t *flags6, int n_turns, int cap, int32_t *tokens_out, uint8_t *is_action_out, float *reward_out,
                                     int *done_out) {
    if (!tokens || !guess6 || !obs6 || !reward6 || !flags6 || !tokens_out || !is_action_out || !reward_out || cap <= 0 || n_turns < 0 ||
        n_turns > kWordleTries || tokens->n_header < 0 || tokens->n_header > 8)
        return -1;
    WordleEpisode ep;
    ep.n_turns = n_turns;
    for (int k = 0; k < kWordleTries; k++) {
        ep.guess[k] = k < n_turns ? guess6[k] : 0u;
        ep.obs[k] = k < n_turns ? obs6[k] : 0u;
        ep.reward[k] = k < n_turns ? reward6[k] : 0.f;
    }
    const int nt = wordle_episode_ntok(*tokens, ep);
    if (nt > cap) return -1;
    for (int s = 0; s < cap; s++) {
        int32_t tok = tokens->pad; uint8_t ia = 0; float rw = 0.f;
        wordle_episode_slot(*tokens, ep, s, tok, ia, rw);
        tokens_out[s] = tok; is_action_out[s] = ia; reward_out[s] = rw;
    }
    if (done_out) *done_out = (n_turns > 0 && (flags6[n_turns - 1] & 1u)) ? 1 : 0;
    return nt;
}

int lmrl_offline_block(const lmrl_ppo_records *rec, const int32_t *keep_d, int n_keep, int max_len, int pad, int truncate_left, const float *returns_d,
                       int returns_pitch, const lmrl_offline_blocks *out, void *stream) {
    LMRL_REQUIRE(records_ok(rec) && out && out->input_ids && out->lengths && max_len >= 2, "lmrl_offline_block: bad argument");
    LMRL_REQUIRE((!keep_d || n_keep > 0) && (!out->returns || (returns_d && returns_pitch > 0)), "lmrl_offline_block: bad argument");
    const int m = keep_d ? n_keep : rec->n;
    hipLaunchKernelGGL(offline_block_kernel, dim3(ceil_div(m, 4)), dim3(256), 0, as_stream(stream), records_of(rec), keep_d, m, max_len, pad, truncate_left,
                       returns_d, returns_pitch, *out);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_record_returns(const lmrl_ppo_records *rec, float *returns_d, void *stream) {
    LMRL_REQUIRE(records_ok(rec) && returns_d, "lmrl_record_returns: bad argument");
    hipStream_t s = as_stream(stream);
    LMRL_CHECK_HIP(hipMemsetAsync(returns_d, 0, (size_t)rec->n_chains * sizeof(float), s));
    hipLaunchKernelGGL(record_returns_kernel, dim3(ceil_div(rec->n, 4)), dim3(256), 0, s, records_of(rec), returns_d);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

}  // extern "C"
