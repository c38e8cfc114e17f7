// wordle_policy.hip — scripted Wordle policies and the device-resident episode loop for gfx950.
//
// Replaces, for N episodes in lock-step,
//   RandomMixturePolicy / OptimalPolicy / StartWordPolicy / MixturePolicy   llm_rl_scripts/wordle/env/scripted_policies.py:42-153
//   PolicyDataGenerator's interact_environment loop                          llm_rl_scripts/wordle/env/data.py:9-34
// (scalar logic and the facts it rests on: wordle_policy_core.h).
//
// One act is four launches on one stream:
//   plan    one wave per env: the policy stream's coins, the start word, or the env's filtered list (file order) into scratch
//   scan    one workgroup: exclusive scan of the list lengths -> the flat (env, guess) item space of this turn
//   score   a fixed grid of waves strides over the items: F differs per env by two orders of magnitude, so an item, not an env, is the
//           unit of work.  A wave sweeps the item's F targets 64 at a time into 243 pattern buckets in LDS (count + first occurrence),
//           then adds the groups' terms in first-occurrence order — the float64 sum has the reference's operation order
//   select  one wave per env: max + ties over the env's scores, random.choice on the policy stream; the mixture's word on the env stream
// The all-POSSIBLE state (every first turn without a start word, and every turn after an invalid first word) is the same for all envs:
// it is one extra row of the item space, scored once per scratch buffer.
#include "../../include/lmrl_amd.h"
#include "common.h"
#include "mt19937.h"
#include "wordle_core.h"
#include "wordle_ctx.h"
#include "wordle_policy_core.h"

namespace lmrl {

static_assert(sizeof(lmrl_wordle_policy_desc) == 16 + 2 * 24 + 4 * kWordleMaxStartWords, "descriptor layout");
static_assert(LMRL_WORDLE_MAX_START_WORDS == kWordleMaxStartWords && LMRL_WORDLE_POLICY_MIXTURE == kWordlePolMixture &&
              LMRL_WORDLE_POLICY_OPTIMAL == kWordlePolOptimal, "header constants");

enum { MODE_NONE = 0, MODE_DONE = 1, MODE_ALL = 2, MODE_SMART = 3, MODE_OPT = 4, MODE_OPT_INIT = 5 };
enum { HDR_NEED_INIT = 0, HDR_INIT_READY = 1, HDR_WORDS = 16 };

// scratch: gains double[(n+1)*V] | hdr u32[16] | mode u32[n] | flen u32[n+1] | prefix u32[n+2] | filt u16[n*V]
struct PolicyScratch {
    double *gains;
    uint32_t *hdr, *mode, *flen, *prefix;
    uint16_t *filt;
};
static size_t scratch_layout(void *base, int n, int V, PolicyScratch *s) {
    char *p = (char *)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = p ? p + off : nullptr; off += (bytes + 15) & ~(size_t)15; return q; };
    PolicyScratch t;
    t.gains = (double *)take(sizeof(double) * (size_t)(n + 1) * V);
    t.hdr = (uint32_t *)take(sizeof(uint32_t) * HDR_WORDS);
    t.mode = (uint32_t *)take(sizeof(uint32_t) * (size_t)n);
    t.flen = (uint32_t *)take(sizeof(uint32_t) * (size_t)(n + 1));
    t.prefix = (uint32_t *)take(sizeof(uint32_t) * (size_t)(n + 2));
    t.filt = (uint16_t *)take(sizeof(uint16_t) * (size_t)n * V);
    if (s) *s = t;
    return off;
}

__device__ __forceinline__ void load_masks(const uint32_t *st, int n, int e, WordleMasks &s) {
#pragma unroll
    for (int i = 0; i < 5; i++) {
        s.forb[i] = st[(size_t)(ROW_FORB + i) * n + e];
        s.must[i] = st[(size_t)(ROW_MUST + i) * n + e];
    }
    wordle_derive(s);
}

// ---- plan: coins and start words on the policy stream (lane 0), filtered lists by the whole wave
__global__ __launch_bounds__(256) void wordle_policy_plan_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ wmasks, int V,
                                                                 lmrl_wordle_policy_desc desc, const uint32_t *st, void *mt_pol,
                                                                 const uint8_t *active, PolicyScratch sc, uint32_t *guess, int n) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n) return;                               // wave-uniform
    if (active && !active[e]) {
        if (lane == 0) { sc.mode[e] = MODE_NONE; sc.flen[e] = 0; }
        return;
    }
    WordleMasks s;
    load_masks(st, n, e, s);
    uint32_t mode = MODE_NONE;
    if (lane == 0) {
        const MtRef pol = mt_ref(mt_pol, n, e);
        int leaf = 0;
        if (desc.coin) leaf = (mt_random(pol) < desc.prob1) ? 0 : 1;                     // MixturePolicy.act (:151)
        const lmrl_wordle_policy_leaf L = desc.leaf[leaf];
        if (L.kind == kWordlePolMixture) {
            mode = (mt_random(pol) < L.prob_smart) ? MODE_SMART : MODE_ALL;              // RandomMixturePolicy.act (:124)
        } else if (st[(size_t)ROW_NACT * n + e] == 0u && L.n_start > 0) {
            // OptimalPolicy.act (:80-81) -> StartWordPolicy.act (:60-64) on an empty history: every start word is still consistent
            guess[e] = desc.start_words[L.start_off + (int)mt_randbelow(pol, (uint32_t)L.n_start)];
            mode = MODE_DONE;
        } else {
            mode = wordle_is_initial(s) ? MODE_OPT_INIT : MODE_OPT;
        }
    }
    mode = __shfl(mode, 0);
    uint32_t cnt = 0;
    if (mode == MODE_OPT) {
        uint16_t *row = sc.filt + (size_t)e * V;
        for (int base = 0; base < V; base += 64) {
            const int i = base + lane;
            const bool ok = i < V && wordle_consistent(s, words[i], wmasks[i]);
            const unsigned long long b = __ballot(ok);
            if (ok) row[cnt + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)i;
            cnt += (uint32_t)__popcll(b);
        }
    }
    if (lane == 0) {
        sc.mode[e] = mode;
        sc.flen[e] = cnt;
        if (mode == MODE_OPT_INIT) atomicOr(&sc.hdr[HDR_NEED_INIT], 1u);
    }
}

// ---- scan: prefix[r] = first item of row r, rows 0..n (row n = the shared all-POSSIBLE state), prefix[n+1] = number of items
__global__ __launch_bounds__(1024) void wordle_policy_scan_kernel(PolicyScratch sc, int V, int n) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    if (t == 0) sc.flen[n] = (sc.hdr[HDR_NEED_INIT] && !sc.hdr[HDR_INIT_READY]) ? (uint32_t)V : 0u;
    __syncthreads();
    const int rows = n + 1;
    const int per = (rows + 1023) / 1024;
    const int lo = t * per, hi = min(lo + per, rows);
    uint32_t sum = 0;
    for (int r = lo; r < hi; r++) sum += sc.flen[r];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (int r = lo; r < hi; r++) { sc.prefix[r] = run; run += sc.flen[r]; }
    if (t == 1023) sc.prefix[rows] = part[1023];
}

// ---- score: one wave per (row, guess) item
constexpr int kScoreWavesPerBlock = 4;
__global__ __launch_bounds__(256) void wordle_policy_score_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ wmasks, int V,
                                                                  PolicyScratch sc, const double *__restrict__ logtab, int n) {
    __shared__ uint32_t lds_cnt[kScoreWavesPerBlock][256];
    __shared__ uint32_t lds_first[kScoreWavesPerBlock][256];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    uint32_t *cnt = lds_cnt[w], *first = lds_first[w];
    const uint32_t total = sc.prefix[n + 1];
    const uint32_t n_waves = gridDim.x * kScoreWavesPerBlock;
    for (uint32_t item = blockIdx.x * kScoreWavesPerBlock + w; item < total; item += n_waves) {   // wave-uniform
        int lo = 0, hi = n + 1;                        // largest row with prefix[row] <= item (empty rows share a prefix: take the last)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (sc.prefix[mid] <= item) lo = mid; else hi = mid;
        }
        const int row = lo;
        const uint32_t k = item - sc.prefix[row];
        const uint32_t F = sc.flen[row];
        const uint16_t *list = row < n ? sc.filt + (size_t)row * V : nullptr;     // row n: the identity list
        const uint32_t g = words[list ? list[k] : k];
        for (int p = lane; p < 256; p += 64) { cnt[p] = 0u; first[p] = 0xFFFFFFFFu; }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t base = 0; base < F; base += 64) {
            const uint32_t j = base + lane;
            if (j < F) {
                const uint32_t ti = list ? list[j] : j;
                const uint32_t p = wordle_pattern(g, words[ti], wmasks[ti]);
                atomicAdd(&cnt[p], 1u);
                atomicMin(&first[p], j);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        double acc = 0.0;
        for (uint32_t base = 0; base < F; base += 64) {
            const uint32_t j = base + lane;
            uint32_t p = 0;
            bool is_first = false;
            if (j < F) {
                const uint32_t ti = list ? list[j] : j;
                p = wordle_pattern(g, words[ti], wmasks[ti]);
                is_first = first[p] == j;
            }
            unsigned long long b = __ballot(is_first);
            while (b) {                                 // groups in order of first occurrence, the same serial sum in every lane
                const int src = __ffsll((long long)b) - 1;
                b &= b - 1;
                const uint32_t c = cnt[__shfl(p, src)];
                acc = wordle_gain_add(acc, c, c, logtab);
            }
        }
        if (lane == 0) sc.gains[(size_t)row * V + k] = wordle_gain_finish(acc, F, logtab);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- select: the word of every env
__global__ __launch_bounds__(256) void wordle_policy_select_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ wmasks, int V,
                                                                   const uint32_t *st, void *mt_env, void *mt_pol, PolicyScratch sc,
                                                                   uint32_t *guess, uint32_t *diag_f, uint32_t *diag_nbest, double *diag_info,
                                                                   int n) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n) return;
    const uint32_t mode = sc.mode[e];
    if (lane == 0 && mode != MODE_NONE) {
        if (diag_f) diag_f[e] = 0u;
        if (diag_nbest) diag_nbest[e] = 0u;
        if (diag_info) diag_info[e] = 0.0;
    }
    if (mode == MODE_ALL) {                            // vocab.get_random_word_all (game.py:181-182)
        if (lane == 0) guess[e] = words[mt_randbelow(mt_ref(mt_env, n, e), (uint32_t)V)];
    } else if (mode == MODE_SMART) {                   // vocab.get_random_word_filtered (game.py:178-179)
        WordleMasks s;
        load_masks(st, n, e, s);
        uint32_t F = 0;
        for (int base = 0; base < V; base += 64) {
            const int i = base + lane;
            F += (uint32_t)__popcll(__ballot(i < V && wordle_consistent(s, words[i], wmasks[i])));
        }
        uint32_t r = 0;
        if (lane == 0 && F > 0) r = mt_randbelow(mt_ref(mt_env, n, e), F);
        r = __shfl(r, 0);
        uint32_t cnt = 0, pick = kBadGuess;            // F == 0: random.choice([]) raises in the reference; not reachable from reset/step
        for (int base = 0; base < V && F > 0; base += 64) {
            const int i = base + lane;
            const uint32_t wd = i < V ? words[i] : 0u;
            const bool ok = i < V && wordle_consistent(s, wd, wmasks[i]);
            const unsigned long long b = __ballot(ok);
            const uint32_t c = (uint32_t)__popcll(b);
            if (r < cnt + c) {
                const unsigned long long mb = __ballot(ok && (uint32_t)__popcll(b & ((1ull << lane) - 1ull)) == r - cnt);
                pick = __shfl(wd, __ffsll((long long)mb) - 1);
                break;
            }
            cnt += c;
        }
        if (lane == 0) guess[e] = pick;
    } else if (mode == MODE_OPT || mode == MODE_OPT_INIT) {
        const int row = mode == MODE_OPT ? e : n;
        const uint32_t F = mode == MODE_OPT ? sc.flen[e] : (uint32_t)V;
        const double *gains = sc.gains + (size_t)row * V;
        const uint16_t *list = mode == MODE_OPT ? sc.filt + (size_t)e * V : nullptr;
        double best = -__builtin_inf();                // best_info = float('-inf'); `>` replaces, `==` appends (:91-94)
        for (uint32_t k = lane; k < F; k += 64) best = gains[k] > best ? gains[k] : best;
        for (int d = 32; d; d >>= 1) {
            const double o = __shfl_xor(best, d);
            best = o > best ? o : best;
        }
        uint32_t ties = 0;
        for (uint32_t base = 0; base < F; base += 64) {
            const uint32_t k = base + lane;
            ties += (uint32_t)__popcll(__ballot(k < F && gains[k] == best));
        }
        uint32_t r = 0;
        if (lane == 0 && ties > 0) r = mt_randbelow(mt_ref(mt_pol, n, e), ties);       // random.choice(best_words) (:96)
        r = __shfl(r, 0);
        uint32_t cnt = 0, pick = kBadGuess;
        for (uint32_t base = 0; base < F && ties > 0; base += 64) {
            const uint32_t k = base + lane;
            const bool ok = k < F && gains[k] == best;
            const unsigned long long b = __ballot(ok);
            const uint32_t c = (uint32_t)__popcll(b);
            if (r < cnt + c) {
                const unsigned long long mb = __ballot(ok && (uint32_t)__popcll(b & ((1ull << lane) - 1ull)) == r - cnt);
                const uint32_t kk = base + (uint32_t)(__ffsll((long long)mb) - 1);
                pick = words[list ? list[kk] : kk];
                break;
            }
            cnt += c;
        }
        if (lane == 0) {
            guess[e] = pick;
            if (diag_f) diag_f[e] = F;
            if (diag_nbest) diag_nbest[e] = ties;
            if (diag_info) diag_info[e] = best;
        }
    }
}

// the shared row was scored by this act: keep it for every later one on this scratch buffer
__global__ void wordle_policy_commit_kernel(PolicyScratch sc) {
    if (sc.hdr[HDR_NEED_INIT]) sc.hdr[HDR_INIT_READY] = 1u;
    sc.hdr[HDR_NEED_INIT] = 0u;
}

__global__ void wordle_policy_advance_kernel(const uint8_t *flags, uint8_t *active, int32_t *n_turns, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || !active[e]) return;
    n_turns[e] += 1;
    if (flags[e] & 1) active[e] = 0;
}

static bool desc_ok(const lmrl_wordle_policy_desc *d) {
    if (!d) return false;
    for (int l = 0; l < (d->coin ? 2 : 1); l++) {
        const lmrl_wordle_policy_leaf &L = d->leaf[l];
        if (L.kind != kWordlePolMixture && L.kind != kWordlePolOptimal) return false;
        if (L.n_start < 0 || L.start_off < 0 || L.start_off + L.n_start > kWordleMaxStartWords) return false;
    }
    return true;
}
static bool desc_has_optimal(const lmrl_wordle_policy_desc *d) {
    return d->leaf[0].kind == kWordlePolOptimal || (d->coin && d->leaf[1].kind == kWordlePolOptimal);
}

static int policy_act(lmrl_wordle_ctx *ctx, const lmrl_wordle_policy_desc *desc, const void *state_d, void *mt_env_d, void *mt_policy_d,
                      const uint8_t *active_d, const double *logtab_d, const PolicyScratch &sc, uint32_t *guess_d, uint32_t *diag_f_d,
                      uint32_t *diag_nbest_d, double *diag_info_d, int n, hipStream_t stream) {
    const int V = ctx->V;
    hipLaunchKernelGGL(wordle_policy_plan_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, stream, ctx->words_d, ctx->wmask_d, V, *desc,
                       (const uint32_t *)state_d, mt_policy_d, active_d, sc, guess_d, n);
    LMRL_CHECK_LAUNCH();
    if (desc_has_optimal(desc)) {
        hipLaunchKernelGGL(wordle_policy_scan_kernel, dim3(1), dim3(1024), 0, stream, sc, V, n);
        LMRL_CHECK_LAUNCH();
        // enough waves to fill the chip (256 CUs x 8 waves); an item costs O(F), and neighbouring items of one env go to different waves
        const long max_items = (long)(n + 1) * V;
        const int blocks = (int)(max_items / kScoreWavesPerBlock < 1024 ? ceil_div(max_items, kScoreWavesPerBlock) : 1024);
        hipLaunchKernelGGL(wordle_policy_score_kernel, dim3(blocks), dim3(256), 0, stream, ctx->words_d, ctx->wmask_d, V, sc, logtab_d, n);
        LMRL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(wordle_policy_select_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, stream, ctx->words_d, ctx->wmask_d, V,
                       (const uint32_t *)state_d, mt_env_d, mt_policy_d, sc, guess_d, diag_f_d, diag_nbest_d, diag_info_d, n);
    LMRL_CHECK_LAUNCH();
    if (desc_has_optimal(desc)) {
        hipLaunchKernelGGL(wordle_policy_commit_kernel, dim3(1), dim3(1), 0, stream, sc);
        LMRL_CHECK_LAUNCH();
    }
    return LMRL_OK;
}

// ---- host faces
static WordleMasks masks_from(const uint32_t *m) {
    WordleMasks s;
    for (int i = 0; i < 5; i++) { s.forb[i] = m[i]; s.must[i] = m[5 + i]; }
    wordle_derive(s);
    return s;
}

}  // namespace lmrl

using namespace lmrl;

extern "C" {

size_t lmrl_wordle_policy_scratch_bytes(int n, int n_words) {
    if (n <= 0 || n_words <= 0) return 0;
    return scratch_layout(nullptr, n, n_words, nullptr);
}

int lmrl_wordle_policy_act(lmrl_wordle_ctx *ctx, const lmrl_wordle_policy_desc *desc, const void *state_d, void *mt_env_d,
                           void *mt_policy_d, const uint8_t *active_d, const double *logtab_d, void *scratch_d, size_t scratch_bytes,
                           uint32_t *guess_d, uint32_t *diag_f_d, uint32_t *diag_nbest_d, double *diag_info_d, int n, void *stream) {
    LMRL_REQUIRE(ctx && state_d && mt_env_d && mt_policy_d && logtab_d && scratch_d && guess_d && n >= 0, "lmrl_wordle_policy_act: null pointer or negative n");
    LMRL_REQUIRE(desc_ok(desc), "lmrl_wordle_policy_act: bad policy descriptor");
    LMRL_REQUIRE(ctx->V <= 65535, "lmrl_wordle_policy_act: vocabulary above 65535 words");
    if (n == 0) return LMRL_OK;
    PolicyScratch sc;
    LMRL_REQUIRE(scratch_layout(scratch_d, n, ctx->V, &sc) <= scratch_bytes, "lmrl_wordle_policy_act: scratch smaller than lmrl_wordle_policy_scratch_bytes");
    return policy_act(ctx, desc, state_d, mt_env_d, mt_policy_d, active_d, logtab_d, sc, guess_d, diag_f_d, diag_nbest_d, diag_info_d, n, as_stream(stream));
}

int lmrl_wordle_policy_episodes(lmrl_wordle_ctx *ctx, const lmrl_wordle_policy_desc *desc, void *state_d, void *mt_env_d, void *mt_policy_d,
                                const uint64_t *env_seeds_d, const uint64_t *policy_seeds_d, const double *logtab_d, void *scratch_d,
                                size_t scratch_bytes, uint8_t *active_d, uint32_t *rec_guess_d, uint32_t *rec_obs_d, float *rec_reward_d,
                                uint8_t *rec_flags_d, int32_t *n_turns_d, int n, void *stream) {
    LMRL_REQUIRE(ctx && state_d && mt_env_d && mt_policy_d && env_seeds_d && policy_seeds_d && logtab_d && scratch_d && active_d && rec_guess_d &&
                 rec_obs_d && rec_reward_d && rec_flags_d && n_turns_d && n >= 0, "lmrl_wordle_policy_episodes: null pointer or negative n");
    LMRL_REQUIRE(desc_ok(desc), "lmrl_wordle_policy_episodes: bad policy descriptor");
    LMRL_REQUIRE(ctx->V <= 65535, "lmrl_wordle_policy_episodes: vocabulary above 65535 words");
    if (n == 0) return LMRL_OK;
    PolicyScratch sc;
    LMRL_REQUIRE(scratch_layout(scratch_d, n, ctx->V, &sc) <= scratch_bytes, "lmrl_wordle_policy_episodes: scratch smaller than lmrl_wordle_policy_scratch_bytes");
    hipStream_t s = as_stream(stream);
    int rc = lmrl_wordle_reset(ctx, state_d, mt_env_d, env_seeds_d, nullptr, n, stream);
    if (rc) return rc;
    rc = lmrl_mt_seed(mt_policy_d, policy_seeds_d, nullptr, n, stream);
    if (rc) return rc;
    const size_t rows = (size_t)kWordleTries * n;
    LMRL_CHECK_HIP(hipMemsetAsync(rec_guess_d, 0xFF, rows * sizeof(uint32_t), s));
    LMRL_CHECK_HIP(hipMemsetAsync(rec_obs_d, 0, rows * sizeof(uint32_t), s));
    LMRL_CHECK_HIP(hipMemsetAsync(rec_reward_d, 0, rows * sizeof(float), s));
    LMRL_CHECK_HIP(hipMemsetAsync(rec_flags_d, 0, rows, s));
    LMRL_CHECK_HIP(hipMemsetAsync(n_turns_d, 0, (size_t)n * sizeof(int32_t), s));
    LMRL_CHECK_HIP(hipMemsetAsync(active_d, 1, (size_t)n, s));
    for (int t = 0; t < kWordleTries; t++) {
        const size_t o = (size_t)t * n;
        rc = policy_act(ctx, desc, state_d, mt_env_d, mt_policy_d, active_d, logtab_d, sc, rec_guess_d + o, nullptr, nullptr, nullptr, n, s);
        if (rc) return rc;
        rc = lmrl_wordle_step(ctx, state_d, mt_env_d, rec_guess_d + o, active_d, rec_obs_d + o, rec_reward_d + o, rec_flags_d + o, n, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(wordle_policy_advance_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, rec_flags_d + o, active_d, n_turns_d, n);
        LMRL_CHECK_LAUNCH();
    }
    return LMRL_OK;
}

void lmrl_wordle_policy_host_seed(uint32_t *mt, uint64_t seed) {
    uint32_t table[kMtN];
    mt_init_table(table);
    mt_seed(mt_ref(mt, 1, 0), seed, table);
}
double lmrl_wordle_policy_host_random(uint32_t *mt) { return mt_random(mt_ref(mt, 1, 0)); }
uint32_t lmrl_wordle_policy_host_randbelow(uint32_t *mt, uint32_t n) { return mt_randbelow(mt_ref(mt, 1, 0), n); }

int lmrl_wordle_policy_host_apply_feedback(uint32_t *masks10, uint32_t guess, uint32_t obs_code) {
    if (!masks10 || guess == kBadGuess) return LMRL_ERR_ARG;
    WordleMasks s = masks_from(masks10);
    if (!wordle_apply_feedback(s, guess, obs_code)) return LMRL_ERR_ARG;
    for (int i = 0; i < 5; i++) { masks10[i] = s.forb[i]; masks10[5 + i] = s.must[i]; }
    return LMRL_OK;
}

int lmrl_wordle_policy_host_filtered(const uint32_t *words, int n_words, const uint32_t *masks10, int32_t *idx_out) {
    if (!words || !masks10 || !idx_out || n_words <= 0) return -1;
    return wordle_filtered_list(masks_from(masks10), words, n_words, idx_out);
}

int lmrl_wordle_policy_host_gains(const uint32_t *words, int n_words, const uint32_t *masks10, const double *logtab, int stride, int literal,
                                  double *gains_out, int32_t *idx_out) {
    if (!words || !masks10 || !logtab || !gains_out || !idx_out || n_words <= 0 || stride <= 0) return -1;
    const WordleMasks s = masks_from(masks10);
    const int F = wordle_filtered_list(s, words, n_words, idx_out);
    WordleGroup *groups = literal ? new WordleGroup[F > 0 ? F : 1] : nullptr;
    for (int k = 0; k < F; k += stride)
        gains_out[k] = literal ? wordle_gain_literal(s, words[idx_out[k]], words, n_words, idx_out, F, logtab, groups)
                               : wordle_gain_buckets(words[idx_out[k]], words, idx_out, F, logtab);
    delete[] groups;
    return F;
}

uint32_t lmrl_wordle_policy_host_act(const lmrl_wordle_policy_desc *desc, const uint32_t *words, int n_words, const uint32_t *masks10,
                                     int n_actions, const double *logtab, uint32_t *mt_env, uint32_t *mt_policy, int32_t *f_out,
                                     int32_t *n_best_out, int32_t *best_idx_out, double *best_info_out) {
    if (f_out) *f_out = 0;
    if (n_best_out) *n_best_out = 0;
    if (best_info_out) *best_info_out = 0.0;
    if (!desc_ok(desc) || !words || !masks10 || !logtab || !mt_env || !mt_policy || n_words <= 0) return kBadGuess;
    const WordleMasks s = masks_from(masks10);
    const MtRef pol = mt_ref(mt_policy, 1, 0), env = mt_ref(mt_env, 1, 0);
    int leaf = 0;
    if (desc->coin) leaf = (mt_random(pol) < desc->prob1) ? 0 : 1;
    const lmrl_wordle_policy_leaf &L = desc->leaf[leaf];
    int32_t *idx = new int32_t[n_words];
    uint32_t g = kBadGuess;
    if (L.kind == kWordlePolMixture) {
        if (mt_random(pol) < L.prob_smart) {
            const int F = wordle_filtered_list(s, words, n_words, idx);
            if (F > 0) g = words[idx[mt_randbelow(env, (uint32_t)F)]];
        } else {
            g = words[mt_randbelow(env, (uint32_t)n_words)];
        }
    } else if (n_actions == 0 && L.n_start > 0) {
        g = desc->start_words[L.start_off + (int)mt_randbelow(pol, (uint32_t)L.n_start)];
    } else {
        const int F = wordle_filtered_list(s, words, n_words, idx);
        double best = -__builtin_inf();
        int n_best = 0;
        int32_t *best_idx = new int32_t[F > 0 ? F : 1];
        for (int k = 0; k < F; k++) {
            const double gain = wordle_gain_buckets(words[idx[k]], words, idx, F, logtab);
            if (gain > best) { best = gain; n_best = 0; best_idx[n_best++] = idx[k]; }
            else if (gain == best) best_idx[n_best++] = idx[k];
        }
        if (n_best > 0) g = words[best_idx[mt_randbelow(pol, (uint32_t)n_best)]];
        if (f_out) *f_out = F;
        if (n_best_out) *n_best_out = n_best;
        if (best_info_out) *best_info_out = best;
        if (best_idx_out) for (int k = 0; k < n_best; k++) best_idx_out[k] = best_idx[k];
        delete[] best_idx;
    }
    delete[] idx;
    return g;
}
}
