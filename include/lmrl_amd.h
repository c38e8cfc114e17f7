/*
 * lmrl_amd.h — C ABI of liblmrl_amd.so, the MI355X (gfx950) engine behind LMRL-Gym's
 * rollout-and-train hot path.
 *
 * The reference has no FFI: its boundary is the Python protocol in LLM_RL/environment.py and
 * the duck-typed algorithm objects.  The entry points below are what a
 * ctypes binding on the reference side would call (INTEGRATION.md shows the stubs); each
 * one cites the reference code it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - every `*_d` / "device" pointer is HBM owned by the CALLER (e.g. a torch tensor);
 *     contexts (`lmrl_*_ctx`) own only small read-only tables.
 *   - `stream` is a hipStream_t passed as void*; NULL = the null stream.  All calls are
 *     asynchronous with respect to the host unless stated otherwise.
 *   - return value: 0 = ok, non-zero = error (text via lmrl_last_error()).
 *   - batched state is struct-of-arrays over the env index so that lane i touches
 *     consecutive addresses (coalesced HBM access); layouts are documented next to the
 *     *_bytes() function that sizes them.
 */
#ifndef LMRL_AMD_H
#define LMRL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMRL_OK 0
#define LMRL_ERR_ARG 1
#define LMRL_ERR_HIP 2

const char *lmrl_last_error(void);
int lmrl_version(void);
/* Name of the device the library is running on (hipDeviceProp.gcnArchName), "" if none. */
const char *lmrl_device_arch(void);

/* ------------------------------------------------------------------------------------------
 * MT19937 streams — CPython `random.Random(seed)` bit-for-bit.
 * Replaces: wordle/env/env.py:53 (`vocab.rng = random.Random(seed)`), wordle/env/game.py:178-179
 * (`rng.choice`), maze/env/env.py:187-212 + randomness.py:9-19 (`random.seed` / `random.choice`).
 *
 * Layout of an mt buffer for N streams (uint32):  mt[624][N] then idx[N]   -> 625*N*4 bytes.
 * ------------------------------------------------------------------------------------------ */
size_t lmrl_mt_bytes(int n);
/* seed streams where mask_d[i] != 0 (mask_d NULL = all). seeds_d[i] = |seed| as uint64
 * (key length 1 if < 2^32 else 2, exactly as CPython's init_by_array over 32-bit limbs). */
int lmrl_mt_seed(void *mt_d, const uint64_t *seeds_d, const uint8_t *mask_d, int n, void *stream);
/* test hook: out_d[k*n + i] = k-th genrand_uint32 of stream i, k < n_out (advances the streams). */
int lmrl_mt_stream(void *mt_d, uint32_t *out_d, int n_out, int n, void *stream);
/* test hook: out_d[k*n + i] = _randbelow(bounds_d[k]) of stream i (random.Random.choice index). */
int lmrl_mt_randbelow(void *mt_d, const uint32_t *bounds_d, uint32_t *out_d, int n_draws, int n, void *stream);

/* ------------------------------------------------------------------------------------------
 * Batched Wordle MDP — replaces WordleEnvironment / WordleGame / Vocabulary / WordleState
 * (wordle/env/env.py:39-55, wordle/env/game.py:53-296) stepped in lock-step for N envs.
 *
 * Game-state buffer for N envs (uint32, SoA):
 *   forb[5][N]  bit c set  <=> letter c is NOT_HERE at position i   (game.py:17-20 CharKnowledge)
 *   must[5][N]  bit c set  <=> letter c is HERE at position i       (neither bit = POSSIBLE)
 *   n_filtered[N]           len(vocab.filtered_vocab)
 *   n_actions[N]            len(action_history)
 *   hist[6][N]              packed guesses (5 x 5 bit letters), 0xFFFFFFFF = not a 5-letter a-z string
 * -> 19*N*4 bytes.
 * ------------------------------------------------------------------------------------------ */
typedef struct lmrl_wordle_ctx lmrl_wordle_ctx;

#define LMRL_WORDLE_BAD_GUESS 0xFFFFFFFFu /* guess word that is not 5 letters a-z (game.py:214) */
/* pack 5 letters 'a'..'z': sum (c_i - 'a') << (5*i) */

/* words5: V*5 bytes, file order (Vocabulary.from_file, game.py:163-170). Host pointer. */
lmrl_wordle_ctx *lmrl_wordle_create(const char *words5, int n_words, int require_words_in_vocab,
                                    float bad_word_reward);
void lmrl_wordle_destroy(lmrl_wordle_ctx *ctx);
size_t lmrl_wordle_state_bytes(int n);
/* WordleEnvironment.reset for envs with mask_d[i] != 0 (NULL = all): seeds the env's stream in mt_d
 * (env.py:53) and sets the all-POSSIBLE state with filtered_vocab = all_vocab (game.py:208-211). */
int lmrl_wordle_reset(lmrl_wordle_ctx *ctx, void *state_d, void *mt_d, const uint64_t *seeds_d,
                      const uint8_t *mask_d, int n, void *stream);
/*
 * One env.step for every env with active_d[i] != 0 (NULL = all)  (env.py:46-50 -> game.py:213-222).
 *   guess_d[i]  packed guess or LMRL_WORDLE_BAD_GUESS
 *   obs_d[i]    bits [3k,3k+3) k<5: 0 none / 1 'g' / 2 'y' / 3 'b' (transition_sequence()[-1], game.py:273-288);
 *               bits [16,19): number of symbols (0 for an invalid action -> observation text "\n")
 *   reward_d[i] -1 / 0 (int in the reference) or bad_word_reward (game.py:290-293)
 *   flags_d[i]  bit0 done (game.py:295-296), bit1 a target was drawn (valid transition),
 *               bit2 reward is the float bad_word_reward,
 *               bit3 `rng.choice(filtered_vocab)` was reached with an EMPTY filtered vocabulary: the reference raises IndexError
 *                    there (game.py:178-179, 219); the env is marked done and the Python face raises IndexError (unreachable from a
 *                    state produced by reset/step: the sampled target always stays in its own filtered list)
 * Inactive envs: outputs untouched, state untouched.
 */
int lmrl_wordle_step(lmrl_wordle_ctx *ctx, void *state_d, void *mt_d, const uint32_t *guess_d,
                     const uint8_t *active_d, uint32_t *obs_d, float *reward_d, uint8_t *flags_d, int n,
                     void *stream);
/* Kernel form of lmrl_wordle_step: 0 (default) = by batch size — one wavefront per env for the lock-step rollout batches (the 64 lanes sweep
 * the vocabulary together), one LANE per env for env-only workloads from 65 536 envs up (262 144 with a vocabulary above 1024 words): every
 * state access of a wave is one coalesced line, no cross-lane work; 1 / 2 force either.  Both forms are bit-identical (tests/test_gpu_envs.py). */
int lmrl_wordle_set_variant(lmrl_wordle_ctx *ctx, int variant);
/* Export the knowledge state as the reference's 26x5 trits (0 NOT_HERE / 1 POSSIBLE / 2 HERE) + counts. */
int lmrl_wordle_export_state(const void *state_d, uint8_t *trits_d /* [N][26][5] */,
                             uint32_t *n_filtered_d, uint32_t *n_actions_d, int n, void *stream);

/* ------------------------------------------------------------------------------------------
 * Scripted Wordle policies and the device-resident episode loop — replaces RandomMixturePolicy, OptimalPolicy (with an
 * optional StartWordPolicy on the first turn) and MixturePolicy (wordle/env/scripted_policies.py:42-153) and the
 * interact_environment loop of PolicyDataGenerator (wordle/env/data.py:9-34) for N episodes in lock-step.
 *
 * Every episode has two MT19937 streams: the ENV stream (random.Random(env_seed): the env's targets and, as in
 * wordle/misc/data_gen.py where policy and env share one Vocabulary, the words RandomMixturePolicy draws) and the POLICY
 * stream (random.Random(policy_seed), standing for the module-level generator: the mixture coins and every random.choice of
 * OptimalPolicy / StartWordPolicy).  OptimalPolicy is the reference policy with an empty cache at the start of every episode.
 * ------------------------------------------------------------------------------------------ */
#define LMRL_WORDLE_POLICY_MIXTURE 0 /* RandomMixturePolicy(prob_smart) */
#define LMRL_WORDLE_POLICY_OPTIMAL 1 /* OptimalPolicy, n_start > 0: StartWordPolicy(start words) answers the first turn */
#define LMRL_WORDLE_MAX_START_WORDS 64
typedef struct {
    int32_t kind;       /* LMRL_WORDLE_POLICY_* */
    int32_t n_start;    /* OPTIMAL: number of start words (0 = no start-word policy) */
    int32_t start_off;  /* first start word in start_words[] */
    int32_t pad_;
    double prob_smart;  /* MIXTURE */
} lmrl_wordle_policy_leaf;
typedef struct {
    int32_t coin;       /* 1: MixturePolicy(prob1, leaf[0], leaf[1]); 0: leaf[0] alone */
    int32_t pad_;
    double prob1;
    lmrl_wordle_policy_leaf leaf[2];
    uint32_t start_words[LMRL_WORDLE_MAX_START_WORDS]; /* packed; need not be vocabulary words */
} lmrl_wordle_policy_desc;

/* Caller-owned scratch for n envs on a V-word list (filtered lists, info gains, the work-item scan).  ZERO it once after
 * allocation: it also caches the scores of the all-POSSIBLE state, which are the same for every env and every later call on
 * the same ctx / logtab, so that first-turn sweep (V^2 pattern evaluations) runs once per scratch buffer. */
size_t lmrl_wordle_policy_scratch_bytes(int n, int n_words);
/*
 * One policy.act for every env with active_d[i] != 0 (NULL = all).  Reads the knowledge masks and n_actions of state_d (n_filtered
 * is recomputed, so a state rebuilt from text needs those 11 rows only).
 *   logtab_d   double[V + 1], logtab[k] = math.log(k) as the HOST computes it (k >= 1; entry 0 unused) — no device log
 *   guess_d    packed guesses, the layout lmrl_wordle_step takes; inactive envs untouched
 *   diag_*     optional (NULL): per env that computed an OptimalPolicy turn, F, len(best_words) and best_info; 0 elsewhere
 */
int lmrl_wordle_policy_act(lmrl_wordle_ctx *ctx, const lmrl_wordle_policy_desc *desc, const void *state_d, void *mt_env_d,
                           void *mt_policy_d, const uint8_t *active_d, const double *logtab_d, void *scratch_d,
                           size_t scratch_bytes, uint32_t *guess_d, uint32_t *diag_f_d, uint32_t *diag_nbest_d,
                           double *diag_info_d, int n, void *stream);
/*
 * n whole episodes without a host round trip: reset (both streams seeded), then up to 6 x (act, step) with per-env done masking.
 * Records, [6][n] each, rows of turns an env did not play keep guess = LMRL_WORDLE_BAD_GUESS, obs = 0, reward = 0, flags = 0:
 *   rec_guess_d / rec_obs_d / rec_reward_d / rec_flags_d   what lmrl_wordle_policy_act chose and lmrl_wordle_step returned
 *   n_turns_d[n]                                           turns played
 * active_d is a uint8[n] work buffer.  All launches go to `stream` (graph-capturable after one warm call).
 */
int lmrl_wordle_policy_episodes(lmrl_wordle_ctx *ctx, const lmrl_wordle_policy_desc *desc, void *state_d, void *mt_env_d,
                                void *mt_policy_d, const uint64_t *env_seeds_d, const uint64_t *policy_seeds_d,
                                const double *logtab_d, void *scratch_d, size_t scratch_bytes, uint8_t *active_d,
                                uint32_t *rec_guess_d, uint32_t *rec_obs_d, float *rec_reward_d, uint8_t *rec_flags_d,
                                int32_t *n_turns_d, int n, void *stream);
/* Host faces of csrc/wordle_policy_core.h (no device): the functions the kernels run, for the CPU test tier.
 *   words: uint32[V] packed vocabulary in file order; masks10: forb[5] then must[5]; mt: uint32[625] host stream (n = 1 layout) */
void lmrl_wordle_policy_host_seed(uint32_t *mt, uint64_t seed);
double lmrl_wordle_policy_host_random(uint32_t *mt);
uint32_t lmrl_wordle_policy_host_randbelow(uint32_t *mt, uint32_t n);
/* transition_from_str for one action (obs code as lmrl_wordle_step writes it); LMRL_ERR_ARG if it does not hold 5 symbols */
int lmrl_wordle_policy_host_apply_feedback(uint32_t *masks10, uint32_t guess, uint32_t obs_code);
/* filtered list (indices into words) -> returns F */
int lmrl_wordle_policy_host_filtered(const uint32_t *words, int n_words, const uint32_t *masks10, int32_t *idx_out);
/* info gain of every stride-th word of the filtered list (gains_out[k], k % stride == 0); literal != 0: by the reference's literal
 * definition (next states compared as states, sizes counted over the whole vocabulary) instead of the pattern buckets. Returns F. */
int lmrl_wordle_policy_host_gains(const uint32_t *words, int n_words, const uint32_t *masks10, const double *logtab, int stride,
                                  int literal, double *gains_out, int32_t *idx_out);
/* one policy.act on host streams; best_idx_out (int32[V], nullable) receives best_words as vocabulary indices. *n_best_out = 0 when
 * no OptimalPolicy turn was computed.  Returns the packed guess. */
uint32_t lmrl_wordle_policy_host_act(const lmrl_wordle_policy_desc *desc, const uint32_t *words, int n_words,
                                     const uint32_t *masks10, int n_actions, const double *logtab, uint32_t *mt_env,
                                     uint32_t *mt_policy, int32_t *f_out, int32_t *n_best_out, int32_t *best_idx_out,
                                     double *best_info_out);

/* ------------------------------------------------------------------------------------------
 * Batched Maze MDP — replaces MazeEnv.reset/step, update_position and the reward functions
 * (maze/env/env.py:104-131,161-214).  Text rendering of observations stays on the host.
 *
 * State buffer for N envs (int32, SoA): pos_r[N] pos_c[N] goal_r[N] goal_c[N] num_steps[N] -> 20*N bytes.
 * ------------------------------------------------------------------------------------------ */
typedef struct lmrl_maze_ctx lmrl_maze_ctx;

#define LMRL_MAZE_LEFT 0   /* 'move left\n'  (0,-1)   env.py:94-99 */
#define LMRL_MAZE_RIGHT 1  /* 'move right\n' (0,+1) */
#define LMRL_MAZE_UP 2     /* 'move up\n'    (-1,0) */
#define LMRL_MAZE_DOWN 3   /* 'move down\n'  (+1,0) */
#define LMRL_MAZE_OTHER 4  /* any other action string */

#define LMRL_MAZE_KIND_OBS 0      /* history + observation, truncated to last_k      env.py:182-184 */
#define LMRL_MAZE_KIND_FAILURE 1  /* (Text("Failure\n"),), -1.0, True                env.py:164-165 */
#define LMRL_MAZE_KIND_SUCCESS 2  /* (Text("Success\n"),), reward, True              env.py:173-174 */
#define LMRL_MAZE_KIND_OBS_ONLY 3 /* illegal action string: history := (observation,) env.py:179-180 */

/* grid: rows*cols bytes (1 = wall); valid_goals: n_goals (row, col) int32 pairs; max_steps < 0 = None;
 * rewards: {at_goal, illegal_action, otherwise} e.g. standard_reward = {0,-4,-1} (env.py:109-115). */
lmrl_maze_ctx *lmrl_maze_create(const uint8_t *grid, int rows, int cols, const int32_t *valid_goals,
                                int n_goals, int max_steps, const float rewards[3]);
void lmrl_maze_destroy(lmrl_maze_ctx *ctx);
size_t lmrl_maze_state_bytes(int n);
/* MazeEnv.reset (env.py:186-214). opt_goal_d / opt_init_d: [N][2] int32, row < 0 = not given (then drawn with
 * random.choice from the env's freshly seeded stream, goal first).  NULL = never given. */
int lmrl_maze_reset(lmrl_maze_ctx *ctx, void *state_d, void *mt_d, const uint64_t *seeds_d,
                    const int32_t *opt_goal_d, const int32_t *opt_init_d, const uint8_t *mask_d, int n,
                    void *stream);
/* MazeEnv.step (env.py:161-184). walls_d: bit0 right, bit1 left, bit2 above, bit3 below (env.py:59). */
int lmrl_maze_step(lmrl_maze_ctx *ctx, void *state_d, const uint8_t *action_d, const uint8_t *active_d,
                   float *reward_d, uint8_t *done_d, uint8_t *kind_d, uint8_t *walls_d, int n, void *stream);

/* ------------------------------------------------------------------------------------------
 * Chess env stepping (csrc/chess.hip, csrc/chess_rules.h): python-chess as the reference's chess env uses it
 * (llm_rl_scripts/chess/env/env.py:28-185 — Board(fen), push_san, san, fen, is_checkmate, is_game_over), one game per lane.
 * The opponent (Stockfish over UCI, env.py:157-170) is a host process pool and hands its moves back in UCI form.
 * Position buffer: lmrl_chess_pos_bytes() per game.  Strings are fixed-pitch, NUL-terminated: FEN LMRL_CHESS_FEN_BYTES, SAN action
 * LMRL_CHESS_ACTION_BYTES, UCI move 8 bytes.
 * ------------------------------------------------------------------------------------------ */
#define LMRL_CHESS_FEN_BYTES 96
#define LMRL_CHESS_ACTION_BYTES 16
#define LMRL_CHESS_ILLEGAL 0   /* unparsable / illegal / ambiguous SAN: reward -1, not done, board unchanged   env.py:109-118 */
#define LMRL_CHESS_MOVED 1     /* legal move, game goes on: the opponent is to move */
#define LMRL_CHESS_GAME_OVER 2 /* legal move ended the game: reward 1 if checkmate else 0, done                env.py:121-125 */
#define LMRL_CHESS_NULL_MOVE 3 /* '--' / 'Z0': reward -1, done                                                env.py:111-113 */
size_t lmrl_chess_pos_bytes(void);
/* chess.Board(fen) for n games; ok_d[i] = 0 for a malformed FEN */
int lmrl_chess_reset(void *pos_d, const char *fens_d, uint8_t *ok_d, int n, void *stream);
/* the agent's half of ChessEnv.step: actions_d [n][LMRL_CHESS_ACTION_BYTES] SAN (blanks already removed); result_d = LMRL_CHESS_*,
 * fen_out_d [n][LMRL_CHESS_FEN_BYTES] = board.fen() after the half-step; uci_out_d [n][8] (optional) = the played move in UCI form (what the
 * engine is told, env.py:121), empty for an illegal action; inactive games: result 255, nothing written */
int lmrl_chess_agent_step(void *pos_d, const char *actions_d, const uint8_t *active_d, float *reward_d, uint8_t *done_d, uint8_t *result_d,
                          char *fen_out_d, char *uci_out_d, int n, void *stream);
/* the opponent's half: uci_d [n][8] a legal engine move; san_out_d = board.san(move) BEFORE it is played (env.py:163), reward -1 if the agent
 * is mated, done = is_game_over(); ok_d = 0 if the move is not legal in the position */
int lmrl_chess_opponent_step(void *pos_d, const char *uci_d, const uint8_t *active_d, float *reward_d, uint8_t *done_d, uint8_t *ok_d, char *san_out_d,
                             char *fen_out_d, int n, void *stream);
/* board.legal_moves (+ board.san of each), board.fen(), is_check / is_checkmate / is_game_over ... of n games in one launch
 * (env.py:157-170 random opponent `random.choice(list(board.legal_moves))`, :150-155 `is_game_over`; chess/eval move-accuracy loops):
 * uci_out_d [n][lmrl_chess_max_moves()][8], san_out_d [n][lmrl_chess_max_moves()][LMRL_CHESS_ACTION_BYTES], count_d [n], status_d [n] with
 * the bits of lmrl_chess_host_status, fen_out_d [n][LMRL_CHESS_FEN_BYTES]; every output is optional (NULL) */
int lmrl_chess_max_moves(void);
int lmrl_chess_describe(const void *pos_d, char *uci_out_d, char *san_out_d, int32_t *count_d, uint8_t *status_d, char *fen_out_d, int n, void *stream);
/* the same rules on ONE position in host memory (CPU-tier tests, oracle comparisons; no GPU needed).  Negative return = bad argument. */
int lmrl_chess_host_from_fen(const char *fen, void *pos);
int lmrl_chess_host_fen(const void *pos, char *out);                                  /* -> length */
int lmrl_chess_host_legal_moves(const void *pos, char *out_uci /* [256][8] */, char *out_san /* [256][16] or NULL */);   /* -> count */
int lmrl_chess_host_agent_step(void *pos, const char *san, float *reward, int *done);  /* -> LMRL_CHESS_* */
int lmrl_chess_host_opponent_step(void *pos, const char *uci, char *san_out, float *reward, int *done);   /* -> 1 if the move was legal */
/* bit0 check, bit1 checkmate, bit2 is_game_over, bit3 insufficient material, bit4 stalemate, bit5 fivefold repetition, bit6 75-move rule */
int lmrl_chess_host_status(const void *pos);

/* ------------------------------------------------------------------------------------------
 * Per-token RL reductions (wavefront-shuffle kernels).
 * ------------------------------------------------------------------------------------------ */
/*
 * GAE over compacted action tokens, one chain per row — get_advantages_and_returns
 * (LLM_RL/algorithms/ppo/base_interface.py:253-293) fed exactly as at :586-606:
 *   values_d  [B][Lv]   per-chain values incl. the bootstrap slot (values_chains, :554-570)
 *   rewards_d [B][L]    per-token rewards (already KL-penalised, :580-584), L = Lv-1
 *   sta_d     [B][L]    should_take_action (uint8)
 *   len_d     [B]       valid length of each chain (<= L)
 * Outputs adv_d/ret_d [B][L]: advantage / return scattered back to action-token positions, 0 elsewhere
 * (:635-645).  The state / next-state pairing is get_action_state_next_state_idxs (:230-243).
 */
int lmrl_gae(const float *values_d, const float *rewards_d, const uint8_t *sta_d, const int32_t *len_d,
             float *adv_d, float *ret_d, int b, int l, float gamma, float lam, void *stream);
/* Reward-to-go over action tokens — get_rtg + MCData scatter (LLM_RL/algorithms/mc_returns/data.py:10-14,49-74). */
int lmrl_rtg(const float *rewards_d, const uint8_t *sta_d, const int32_t *len_d, float *rtg_d, int b, int l,
             float gamma, void *stream);
/* Masked whitening over ALL selected elements of x (ppo/base_interface.py:245-251, :609-615):
 * y = (x-mean)*rsqrt(var+1e-8) (+mean if !shift_mean) where mask, y = x elsewhere. In place allowed.
 * moments_d (3 doubles: sum, sumsq, count) is caller scratch; when `moments_only` != 0 only the local
 * moments are produced (so ranks can all-reduce them) and `lmrl_whiten_apply` finishes the job. */
int lmrl_whiten_moments(const float *x_d, const uint8_t *mask_d, double *moments_d, size_t n, void *stream);
/* The rollout-sized chain GAE -> whiten in two launches instead of four: lmrl_gae_moments = lmrl_gae that also leaves per-workgroup partial moments
 * of the advantages on action slots (partials_d: 3 doubles x lmrl_gae_moments_partials(b, l), 0 = shape not covered: use lmrl_gae +
 * lmrl_whiten_moments); lmrl_whiten_apply_partials adds the partials in a fixed order in every workgroup and applies (one rank); ranks that
 * all-reduce the moments call lmrl_whiten_finish (partials -> the 3 moments) + the collective + lmrl_whiten_apply.  Same numbers as the separate
 * calls up to the fp64 association order of the moments (ppo/base_interface.py:245-293, 609-615). */
int lmrl_gae_moments_partials(int b, int l);
int lmrl_gae_moments(const float *values_d, const float *rewards_d, const uint8_t *sta_d, const int32_t *len_d, float *adv_d, float *ret_d, int b, int l,
                     float gamma, float lam, double *partials_d, void *stream);
int lmrl_whiten_finish(const double *partials_d, int n_partials, double *moments_d, void *stream);
int lmrl_whiten_apply_partials(const float *x_d, const uint8_t *mask_d, const double *partials_d, int n_partials, float *y_d, size_t n, int shift_mean,
                               void *stream);
int lmrl_whiten_apply(const float *x_d, const uint8_t *mask_d, const double *moments_d, float *y_d, size_t n,
                      int shift_mean, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rollout records -> PPO data without leaving the device (csrc/ppo_data.hip).
 * Replaces the host side of PPOInference.get_ppo_data_from_token_trajectory_chain
 * (LLM_RL/algorithms/ppo/base_interface.py:464-669) as the task scripts feed it
 * (llm_rl_scripts/wordle/ppo/train_ppo_gpt2.py:301-353), PPOData.block / PPODataset
 * (LLM_RL/algorithms/ppo/data.py:9-114) and the masks GPT2PPOTrain.step derives from a batch
 * (base_interface.py:172-228).  The forwards between lmrl_ppo_block and lmrl_ppo_shape, lmrl_gae and
 * lmrl_whiten_* between lmrl_ppo_shape and lmrl_ppo_unroll are the caller's.
 * ------------------------------------------------------------------------------------------ */
/* n token trajectories = the fields of TokenTrajectory (LLM_RL/environment.py:329-380) as the rollout engines record
 * them, grouped into n_chains TokenTrajectoryChains (environment.py:383-420).  All pointers are device pointers. */
typedef struct {
    const int32_t *tokens;      /* [n][cap] */
    const uint8_t *is_action;   /* [n][cap] */
    const float *reward;        /* [n][cap] */
    const int32_t *n_tok;       /* [n] tokens of each trajectory (<= cap) */
    const uint8_t *done;        /* [n_chains] `done` of each chain's LAST trajectory (every earlier one must be not done, :310) */
    const int32_t *chain;       /* [n] chain of trajectory k, or NULL: trajectory k is chain k (n_chains == n) */
    const int32_t *pos;         /* [n] where trajectory k starts in its chain's concatenation (sum of earlier len - 1), or NULL: 0 */
    const uint8_t *last;        /* [n] 1 when trajectory k ends its chain, or NULL: all 1 */
    int32_t n, cap, n_chains;
} lmrl_ppo_records;
/* Per trajectory: effective length = min(n_tok, max_len) (max_len <= 0: no truncation; Truncation.RIGHT, :500-512), rows that predict a next
 * token (len - 1) and action tokens (is_action[1:len]), with their exclusive scans.  cnt_d [2n] scratch; off_rows_d / off_act_d [n + 1];
 * meta_d [8] = {rows, action tokens, longest effective length, pad ids found below a length, action tokens CUT by max_len, trajectories that
 * continue a chain but start with an action token, longest chain concatenation (max of pos + len - 1), 0}.  Words 4 and 5 are the two arms of the
 * reference's 'trajectory truncation error' assert (CombinedTokenTrajectoryChain.from_token_trajectory_chain, :318-327): a caller mirrors it by
 * refusing the batch when either is non-zero; word 6 is the `lc` lmrl_ppo_shape / lmrl_ppo_unroll need. */
int lmrl_ppo_count(const lmrl_ppo_records *rec, int max_len, int pad, int32_t *cnt_d, int32_t *off_rows_d, int32_t *off_act_d, int32_t *meta_d,
                   void *stream);
/* block_sequences(Padding.RIGHT, pad) to width tf + initialize_attn_mask_pos_ids + the compacted list of rows k * tf + t (t < len - 1) with
 * their next-token targets (the LM head of token_logprobs_from_logits, :396-403, runs on these rows only): ids / am / pos [n][tf],
 * rows_idx / tgt [meta[0]]. */
int lmrl_ppo_block(const lmrl_ppo_records *rec, int max_len, int pad, int tf, const int32_t *off_rows_d, int32_t *ids_d, uint8_t *am_d, int32_t *pos_d,
                   int32_t *rows_idx_d, int32_t *tgt_d, void *stream);
/* :543-584 + the PPOData rows: logprobs_d / init_logprobs_d [meta[0]] in row-list order, values_d [n][tf].  Writes per chain
 * (concatenated trajectories, row pitch lc / lc + 1, lc >= every chain's length): values incl. the bootstrap slot value * (1 - done), KL-shaped
 * rewards, should_take_action, the chain length; kls_d [meta[1]] = exp(lr) - 1 - lr over the action tokens in trajectory order; and the blocked
 * dataset rows of width tp (>= the longest effective length): ds_ids [n][tp], ds_sta / ds_logprobs / ds_values [n][tp - 1]. */
int lmrl_ppo_shape(const lmrl_ppo_records *rec, int max_len, int tf, const int32_t *off_rows_d, const int32_t *off_act_d, const float *logprobs_d,
                   const float *init_logprobs_d, const float *values_d, float kl_weight, int lc, float *chain_values_d, float *chain_rewards_d,
                   uint8_t *chain_sta_d, int32_t *chain_len_d, float *kls_d, int pad, int tp, int32_t *ds_ids_d, uint8_t *ds_sta_d, float *ds_logprobs_d,
                   float *ds_values_d, void *stream);
/* unroll_arr (:335-343, :635-660): chain rows of advantages / returns [n_chains][lc] back to ds_adv / ds_ret [n][tp - 1] (0 past a length) */
int lmrl_ppo_unroll(const lmrl_ppo_records *rec, int max_len, int tf, int lc, const float *chain_adv_d, const float *chain_ret_d, int tp, float *ds_adv_d,
                    float *ds_ret_d, void *stream);
/* The task scripts' length rule on single-trajectory chains (llm_rl_scripts/wordle/ppo/train_ppo_gpt2.py:323-341, same loop in the chess / maze
 * PPO scripts): while a trajectory has more than three texts (maximal runs of equal is_action flags) and n_tok >= max_len, drop its last two texts,
 * add (sum of their rewards) * gamma to the reward of the previous action (its last token) and clear `done`; keep[k] = 0 for trajectories left
 * with fewer than three texts or still >= max_len tokens (the script's two `continue`s).  reward_d [n][cap] is updated IN PLACE (pass a copy of a
 * rollout engine's record), n_tok_out_d / done_out_d / keep_d [n]; meta_d [2] = {trajectories shortened, trajectories skipped}. */
int lmrl_ppo_truncate_turns(const uint8_t *is_action_d, const int32_t *n_tok_d, const uint8_t *done_d, int n, int cap, int max_len, double gamma,
                            float *reward_d, int32_t *n_tok_out_d, uint8_t *done_out_d, uint8_t *keep_d, int32_t *meta_d, void *stream);
/* idx_d[j] = the j-th index k with flags_d[k] != 0, increasing; count_d[0] = how many (row compaction of a record after lmrl_ppo_truncate_turns:
 * lmrl_gather_rows_bytes by idx_d); one workgroup */
int lmrl_compact_flags(const uint8_t *flags_d, int n, int32_t *idx_d, int32_t *count_d, void *stream);
/* initialize_attn_mask_pos_ids (JaxSeq; call sites base_interface.py:190-195): am = ids != pad, pos = max(cumsum(am) - 1, 0); [b][t].
 * am_next_f32_d (optional) [b][t - 1] = float(am[:, 1:]), the mask ppo_loss_fn multiplies in (base_interface.py:208-214). */
int lmrl_seq_mask_pos(const int32_t *ids_d, int pad, uint8_t *am_d, int32_t *pos_d, float *am_next_f32_d, int b, int t, void *stream);
/* The same two arrays for right-padded rows of KNOWN lengths (am[r][i] = i < len[r]): a device-resident PPO dataset hands the train step the masks its
 * data build used instead of re-deriving them from `ids != pad` (lmrl_gym_amd.algorithms.ppo_device.DevicePPODataset.batch). */
int lmrl_len_mask_pos(const int32_t *len_d, int b, int t, uint8_t *am_d, int32_t *pos_d, void *stream);
/* out[i] = in[i] + c (row-list indices re-based to a chunk of the batch; lengths from row counts) */
int lmrl_add_i32(const int32_t *in_d, int c, int32_t *out_d, int n, void *stream);
/* rows r = row * t + i (i < t - 1) with sta[row][i] && am[row][i + 1] (am NULL: sta alone), increasing, + tgt = ids[row][i + 1] (tgt NULL: no
 * targets) — the rows of [b * t, d] hidden states whose LM-head outputs a masked loss reads.  cnt_d [b] scratch, off_d [b + 1] (off_d[b] = count),
 * idx_d / tgt_d capacity b * (t - 1). */
int lmrl_masked_rows(const uint8_t *sta_d, const uint8_t *am_d, const int32_t *ids_d, int b, int t, int32_t *cnt_d, int32_t *off_d, int32_t *idx_d,
                     int32_t *tgt_d, void *stream);
/* out_d [n + 1] = exclusive prefix sums of in_d [n] (out_d[n] = the total); one workgroup */
int lmrl_exclusive_scan_i32(const int32_t *in_d, int32_t *out_d, int n, void *stream);
/* dst[i] = src[idx[i]] for rows of row_bytes bytes (a shuffled batch of a device-resident dataset: ppo/data.py:88-98) */
int lmrl_gather_rows_bytes(const void *src_d, const int32_t *idx_d, void *dst_d, int n, long row_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * GPT-2 rollout forward with a persistent per-env KV cache (csrc/gpt2.hip).
 * Replaces the model side of GPT2PPOPolicy.act / GPT2ValuePolicy.act
 * (LLM_RL/algorithms/ppo/gpt2/interface.py:507-546, value_rl_base/gpt2/interface.py:281-320), whose
 * transformer lives in JaxSeq / HF-Flax (third party).
 *
 * Engine weight layout (all device pointers, caller-owned):
 *   wte  bf16 [vocab_padded][d]  (rows >= vocab zero)        wpe  bf16 [n_pos][d]
 *   per layer, 12 pointers in this order:
 *     ln1_g f32[d], ln1_b f32[d], w_qkv bf16[3d][d], b_qkv f32[3d], w_proj bf16[d][d], b_proj f32[d],
 *     ln2_g f32[d], ln2_b f32[d], w_fc bf16[dff][d], b_fc f32[dff], w_fc2 bf16[d][dff], b_fc2 f32[d]
 *   i.e. every matrix is stored [out][in] (HF Conv1D weights transposed once at load time).
 * KV cache: bf16 [n_layer][2 (K,V)][B][tmax][n_head*64] (token-major: one env's keys for all heads are one contiguous stream).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_layer, n_head, d_model, d_ff, vocab, vocab_padded, n_pos;
    float ln_eps;
} lmrl_gpt2_config;

typedef struct lmrl_gpt2 lmrl_gpt2;

lmrl_gpt2 *lmrl_gpt2_create(const lmrl_gpt2_config *cfg, const void *wte_d, const void *wpe_d, const float *lnf_g_d,
                            const float *lnf_b_d, const void *const *layer_ptrs /* host array [n_layer*12] */);
void lmrl_gpt2_destroy(lmrl_gpt2 *m);
/* The caller has overwritten the weight tensors handed to lmrl_gpt2_create IN PLACE (the online loops copy the trainer's parameters into the
 * rollout engine after every round: train_ppo_gpt2.py `policy.set_params(...)`): re-derive the model-owned LayerNorm-folded copies on `stream`.
 * Pointers held by sessions and captured hipGraphs stay valid. */
int lmrl_gpt2_refresh(lmrl_gpt2 *m, void *stream);
/*
 * Pinned prefix: the K/V rows (and last hidden state) of a fixed token prefix, held in the cache of a 1-env KV session, as a derived product of
 * the weights — like the LayerNorm-folded copies.  `pin` prefills the prefix once on `stream`: *len_d := 0, then one forward of 1 env x 8 slots
 * per 8 tokens through the code path of lmrl_gpt2_forward with `flags` (the session's LMRL_FWD_* bits), i.e. launch for launch what the
 * session's own reset + chunk forwards would do; the rows are bit-identical to theirs.  The model handle remembers the pin, and
 * lmrl_gpt2_refresh re-runs that prefill for every pin, after the fold kernels, on the stream it is given.  Every writer of the weights
 * already has to call lmrl_gpt2_refresh, so a pinned prefix cannot go stale without the folded weights going stale too; consumers
 * (lmrl_gpt2_kv_broadcast out of the pinned cache, also inside captured hipGraphs) need no prefill of their own.
 * All buffers are the caller's and must stay alive and unchanged in address until lmrl_gpt2_unpin_prefix(kv_d) or lmrl_gpt2_destroy (which
 * drops the list); there is no process-wide state.  kv_d: cache of lmrl_gpt2_kv_bytes(m, 1, tmax); ws_d: lmrl_gpt2_ws_bytes(m, 1, 8), used
 * by pin and by every refresh (its per-env index slot holds the chunk's token count); tokens_d: device int32, READABLE up to the next multiple
 * of 8 entries (the slots past n_tokens are not used); 1 <= n_tokens <= tmax; last_hidden_d optional (bf16 [d]).  A cache can be pinned once
 * (LMRL_ERR_ARG with an lmrl_last_error() text otherwise); unpinning a cache that is not pinned is LMRL_ERR_ARG.
 */
int lmrl_gpt2_pin_prefix(lmrl_gpt2 *m, void *kv_d, int tmax, void *ws_d, const int32_t *tokens_d, int n_tokens, int32_t *len_d,
                         void *last_hidden_d, unsigned flags, void *stream);
int lmrl_gpt2_unpin_prefix(lmrl_gpt2 *m, const void *kv_d);
size_t lmrl_gpt2_kv_bytes(const lmrl_gpt2 *m, int b, int tmax);
size_t lmrl_gpt2_ws_bytes(const lmrl_gpt2 *m, int b, int c);
/*
 * Forward B envs x C token slots (C = 1 decode, C = 8 or 16 chunked prefill).  Env b contributes cnt_d[b] <= C new
 * tokens tokens_d[b*C + j] at positions len_d[b] + j; their K/V rows are appended to the cache and len_d[b] is
 * advanced by cnt_d[b].  last_hidden_d (bf16 [B][d], optional): ln_f of each env's LAST new token (row untouched
 * when cnt_d[b] == 0).  all_hidden_d (bf16 [B*C][d], optional): ln_f of every row.
 * `flags` (LMRL_FWD_*, 0 = defaults) select per-CALL variants; there is no process-wide forward state, so sessions with
 * different settings may be interleaved on any streams.  Every variant computes the same function (the LN-folded and
 * stand-alone paths within bf16 rounding of each other, ragged vs padded bit-identically).
 */
#define LMRL_FWD_LN_STANDALONE 1u  /* stand-alone LayerNorm launches instead of LN folded into the neighbouring GEMMs (A/B, cross-check) */
#define LMRL_FWD_RAGGED_ALWAYS 2u  /* run on the compacted rows (sum of cnt_d) whatever the batch size; default: only when b*c >= 2048 */
#define LMRL_FWD_RAGGED_NEVER  4u  /* always run all b*c slots */
#define LMRL_FWD_ATTN_VALU     8u  /* per-(env, head) multi-round-trip attention kernels instead of the default ones (cross-check) */
#define LMRL_FWD_KV_FROM_GEMM  16u /* decode: the qkv GEMM epilogue appends the new K/V rows, the attention kernel only reads (A/B: attention faster, GEMM slower, net slower) */
#define LMRL_FWD_ATTN_ITEMS2   64u /* decode attention: 2 (env, head) items per wave on a grid of half as many waves (A/B of the resident-size grid; bit-identical) */
#define LMRL_FWD_ATTN_ITEMS3   128u /* ... 3 items per wave */
#define LMRL_FWD_SKINNY       (1u << 30) /* single-token decode of <= 16 sequences: the layer's Dense products on the skinny-M kernels (csrc/skinny_gemm.h: one MFMA row block,
                                          * K split over the waves of a workgroup, every load issued up front) — 7-16 us -> ~3 us per product at 8 rows; same formulas, K summed in
                                          * 8 slices (not bit-identical to the tile kernels: a per-session choice) */
#define LMRL_FWD_FULL_LAST_LAYER 32u /* chunk forwards: run the last layer's projection + MLP on every row (default: only on each env's last new token — the only row whose hidden state is returned; A/B and cross-check, bit-identical) */
/* bits 16-29: reserved — the product library rejects them (LMRL_ERR_ARG). */
#define LMRL_FWD_PRE_EMBEDDED (1u << 31) /* per CALL (c = 1, LN-folded path; not ragged, skinny or prefixed — LMRL_ERR_ARG otherwise): the row embeddings (fp32 and bf16)
                                          * and moment slot 0 of every row are already in ws_d for these tokens_d / cnt_d / len_d (lmrl_wordle_sample_accept_embed wrote
                                          * them): the forward skips its embedding launch.  Bits 0-7 are taken and bits 8-15 carry the shared-prefix length, so the
                                          * switch sits beside LMRL_FWD_SKINNY above the reserved range */
/* bits 8-15: LMRL_FWD_SHARED_PREFIX(n) — positions [0, n) of EVERY env's cache hold the same K/V rows as env 0's (the caller copied them
 * with lmrl_gpt2_kv_broadcast and has not reset the cache since): the decode attention then reads them from env 0 (one L2-resident copy)
 * instead of once per env.  Results are bit-identical; a wrong promise reads env 0's prefix for every env. */
#define LMRL_FWD_SHARED_PREFIX(n) (((unsigned)(n) & 0xffu) << 8)
int lmrl_gpt2_forward(lmrl_gpt2 *m, void *kv_d, int tmax, void *ws_d, const int32_t *tokens_d, const int32_t *cnt_d,
                      int32_t *len_d, int b, int c, void *last_hidden_d, void *all_hidden_d, unsigned flags, void *stream);
/* 1 if a single-token forward of b envs with these session flags (no all_hidden_d, no attached prefix) accepts LMRL_FWD_PRE_EMBEDDED, else 0:
 * the library's own path choice (LN-folded, not ragged, not skinny), for callers that pick between the fused and the three-launch tail. */
int lmrl_gpt2_forward_takes_pre_embedded(const lmrl_gpt2 *m, int b, unsigned flags);

/*
 * Shared prompt prefix: copy positions [0, n_pos) of the single env of a 1-env KV session (src) into all `b` envs of dst,
 * set dst_len_d[i] = n_pos and (optionally) broadcast the prefix's last hidden state.  All envs of a lock-step Wordle batch
 * start from the same header text ('Wordle:\n', wordle/env/env.py:8), so its K/V are computed once per episode instead of
 * once per env; the copied rows are bit-identical to what a per-env forward writes.
 */
int lmrl_gpt2_kv_broadcast(const lmrl_gpt2 *m, const void *src_kv_d, int src_tmax, void *dst_kv_d, int dst_tmax, int b, int n_pos,
                           const void *src_hidden_d, void *dst_hidden_d, int32_t *dst_len_d, void *stream);

/*
 * Prompt-prefix cache (indexed form of lmrl_gpt2_kv_broadcast): env i of dst starts from the prompt held by row idx_d[i] of the session
 * `src` (src_b envs, same model): K/V rows [0, src_len_d[row]), dst_len_d[i] = that length and (optionally) the row's last hidden state.
 * idx_d[i] < 0 leaves env i with an empty cache.  Text envs whose observations form a finite set (Maze with last_k = 1: one prompt per
 * (goal, cell), llm_rl_scripts/maze/env/env.py:8-81,182-184) prefill each distinct prompt once per set of weights instead of once per
 * env per turn (the reference re-encodes and re-runs the whole prompt on every act(), ppo/gpt2/interface.py:519-546); the copied rows are
 * the rows a per-env prefill of the same tokens writes.
 */
int lmrl_gpt2_kv_gather(const lmrl_gpt2 *m, const void *src_kv_d, int src_b, int src_tmax, const int32_t *src_len_d, const void *src_hidden_d,
                        const int32_t *idx_d, void *dst_kv_d, int dst_tmax, int b, void *dst_hidden_d, int32_t *dst_len_d, void *stream);

/*
 * Indexed prompt prefix: the copy-free form of lmrl_gpt2_kv_gather.  lmrl_gpt2_kv_attach sets dst_len_d[i] = pfx_n_d[i] = the prompt length
 * of prefix row idx_d[i] (0 for idx < 0), copies that row's last hidden state and (order_d, optional, [b]) lists the envs grouped by prefix
 * row.  Single-token decode forwards then go through lmrl_gpt2_forward_prefixed: positions [0, n_d[i]) of env i are READ from row row_d[i]
 * of the prefix session's cache — the bytes of a prompt exist once however many envs stand on it, and with order_d each XCD walks envs that
 * share prompts, so those rows are served by its L2 — while the generated tokens' rows go to / come from env i's own cache at their
 * absolute positions.  Results are bit-identical to the copying form (same rows, same order of arithmetic).
 * The reference re-runs the whole prompt per env per act() (ppo/gpt2/interface.py:519-546).
 */
typedef struct {
    const void *kv_d;           /* the prefix session's cache: lmrl_gpt2_kv_bytes(m, n_rows, tmax) */
    int32_t n_rows, tmax;
    const int32_t *row_d;       /* [b] prefix row behind env i (< 0: none) — the idx_d given to lmrl_gpt2_kv_attach */
    const int32_t *n_d;         /* [b] prefix length of env i — pfx_n_d of lmrl_gpt2_kv_attach */
    const int32_t *order_d;     /* [b] launch order (a permutation of the envs) or NULL */
} lmrl_kv_prefix;
int lmrl_gpt2_kv_attach(const lmrl_gpt2 *m, int src_b, const int32_t *src_len_d, const void *src_hidden_d, const int32_t *idx_d, int b,
                        int dst_tmax, void *dst_hidden_d, int32_t *dst_len_d, int32_t *pfx_n_d, int32_t *order_d, void *stream);
int lmrl_gpt2_forward_prefixed(lmrl_gpt2 *m, void *kv_d, int tmax, void *ws_d, const int32_t *tokens_d, const int32_t *cnt_d,
                               int32_t *len_d, int b, void *last_hidden_d, const lmrl_kv_prefix *pfx, unsigned flags, void *stream);

/* C[m][n] = A[m][k] . W[n][k]^T + bias[n]; A, W bf16.  epilogue: 0 bf16, 1 gelu_new->bf16, 2 f32 += (residual),
 * 3 f32, 4 relu->bf16.  Used for the value heads (heads/linear_head.py:112-119, heads/mlp_head.py:139-148). */
int lmrl_gemm_bf16(const void *a_d, const void *w_d, const float *bias_d, void *c_d, int m, int n, int k, int lda,
                   int ldc, int n_store, int epilogue, void *stream);
/* same with an explicit row pitch of W (ldw elements, >= k; 0 = dense): operands whose natural pitch is a large power of two (the
 * transposed operands of the train step's dW products, k = B*T) are padded so that the rows of a tile do not all start in one HBM channel */
int lmrl_gemm_bf16_ld(const void *a_d, const void *w_d, const float *bias_d, void *c_d, int m, int n, int k, int lda, int ldw, int ldc, int n_store,
                      int epilogue, void *stream);
/* c[m][n_store] fp32 = resid[m][..] + a . w^T + bias with the residual operand in ANOTHER buffer (row pitch ldr): the residual add of a
 * transformer block (x_mid = x + attn.c_proj(att), x_out = x_mid + mlp.c_proj(g)) folded into the projection's epilogue when the block's
 * input / middle / output streams are kept as separate tensors — the train step's forward (its LayerNorm backward reads all three). */
int lmrl_gemm_bf16_resid(const void *a_d, const void *w_d, const float *bias_d, const float *resid_d, int ldr, float *c_d, int m, int n, int k, int lda,
                         int ldw, int ldc, int n_store, void *stream);

/* Train step, bf16-matmul mode: Dense products whose epilogue writes the NEXT kernel's bf16 operand, so that no stand-alone elementwise pass
 * re-reads an [B*T][n] fp32 tensor (n a multiple of 128, k of 64; a, w as for lmrl_gemm_bf16_ld).  The HF GPT-2 block the reference differentiates
 * (ppo/gpt2/interface.py:111-133, ilql/gpt2/interface.py:139-177):
 *   gelu_dual : c fp32 [m][ldc] = a . w^T + bias (mlp.c_fc pre-activation, read again by the backward) AND act bf16 [m][ldact] = gelu_new(c)
 *   qkv_heads : attn.c_attn straight into the flash kernels' per-head bf16 matrices q | k | v = [3][batch*heads][pad64(t)][64] (plane_elems
 *               apart, from lmrl_flash_attn_stage_ptrs), q scaled by 1/8; follow with lmrl_flash_attn_finish_staging; m = batch * t rows
 *   gelu_bwd  : c bf16 [m][ldc] = (a . w^T) * gelu_new'(pre[m][n]) — d(pre-activation) of mlp.c_fc as the bf16 dy operand of its backward products */
int lmrl_gemm_bf16_gelu_dual(const void *a_d, const void *w_d, const float *bias_d, float *c_d, int ldc, void *act_bf16_d, int ldact, int m, int n, int k,
                             int lda, int ldw, void *stream);
int lmrl_gemm_bf16_qkv_heads(const void *a_d, const void *w_d, const float *bias_d, void *q_heads_d, long plane_elems, int m, int k, int lda, int ldw,
                             int heads, int t, void *stream);
int lmrl_gemm_bf16_gelu_bwd(const void *a_d, const void *w_d, const float *pre_d, int ldpre, void *c_bf16_d, int ldc, int m, int n, int k, int lda,
                            int ldw, void *stream);
/* The two entries above with the pre-activation stored ROUNDED TO bf16 ([m][ldpre] bf16 elements, ldpre a multiple of 8): the gelu backward is its
 * only reader (ppo/gpt2/interface.py:72-211 and ilql/gpt2/interface.py:88-367 differentiate HF-Flax GPT-2's gelu_new; its bf16 mode keeps every
 * activation in bf16) — half the bytes written by the forward and read by the backward. */
int lmrl_gemm_bf16_gelu_dual_prebf16(const void *a_d, const void *w_d, const float *bias_d, void *pre_bf16_d, int ldpre, void *act_bf16_d, int ldact, int m,
                                     int n, int k, int lda, int ldw, void *stream);
int lmrl_gemm_bf16_gelu_bwd_prebf16(const void *a_d, const void *w_d, const void *pre_bf16_d, int ldpre, void *c_bf16_d, int ldc, int m, int n, int k,
                                    int lda, int ldw, void *stream);

/* Vocabulary-wide heads (the Q heads of ILQL / MC, heads/mlp_head.py:139-148; the tied LM head of PPO) in the bf16-matmul mode: logits written ONCE,
 * in bf16 ([m][ldc], columns [0, n_store)), with everything the cross-entropy / take_along_axis terms need taken from the fp32 accumulators in the
 * same launch — partials_d [m][lmrl_gemm_bf16_ce_slots(m, n, k)] (max, sum exp) pairs -> lmrl_lse_from_partials gives log-sum-exp (and the target's
 * log-probability), tgt_logit_d[r] = logit[r][targets_d[r]] in fp32.  Replaces an fp32 [m][V] logits tensor + a pass over it
 * (optax.softmax_cross_entropy_with_integer_labels forward, ilql/base_interface.py:57-66 gathers).  lmrl_ce_bwd_bf16_inplace then turns the bf16
 * logits into the bf16 d(logits) operand of the head's backward products in place (padding rows / columns zeroed).
 * logits_bf16_d NULL (inference: PPOInference.forward's token log-probabilities, ppo/base_interface.py:396-403): no logits are stored at all. */
int lmrl_gemm_bf16_ce_slots(int m, int n, int k);
int lmrl_gemm_bf16_ce(const void *a_d, const void *w_d, const float *bias_d, void *logits_bf16_d, int ldc, int m, int n, int k, int lda, int ldw, int n_store,
                      const int32_t *targets_d, float *tgt_logit_d, void *partials_d, void *stream);
int lmrl_lse_from_partials(const void *partials_d, int nslots, int rows, const float *tgt_logit_d, float *lse_d, float *logprob_d, void *stream);
int lmrl_ce_bwd_bf16_inplace(void *logits_bf16_d, long ld, int vocab, const float *lse_d, const int32_t *targets_d, const float *coef_ce_d,
                             const float *coef_gather_d, int rows, int rows_dst, void *stream);

/* Split-K form for products with few output tiles and a long K (the train step's weight-gradient products dW = x^T . dy: K = B*T):
 * S copies of the 128 x 128 tile grid each accumulate a slice of K into fp32 partials in ws_d, a fixed-order reduce then writes
 * c (=|+=) their sum — deterministic.  lmrl_gemm_bf16_splitk_ws_bytes returns 0 when the shape is better served by lmrl_gemm_bf16_ld. */
size_t lmrl_gemm_bf16_splitk_ws_bytes(int m, int n, int k);
int lmrl_gemm_bf16_splitk(const void *a_d, const void *w_d, void *c_d, int m, int n, int k, int lda, int ldw, int ldc, int n_store, int accumulate,
                          void *ws_d, void *stream);
/* the same product with a bias and no accumulation, c[m][n] = sum_k a[m][k] w[n][k] + bias[n] (any shape lmrl_gemm_bf16_splitk_ws_bytes has a plan for) — the MLP output
 * projection of the bf16x3 rollout mode at decode size (K' = 3 d_ff = 9216 on 48 tiles) */
int lmrl_gemm_bf16_splitk_bias(const void *a_d, const void *w_d, const float *bias_d, void *c_d, int m, int n, int k, int lda, int ldw, int ldc,
                               void *ws_d, void *stream);

/* The same product on the operands as their producers staged them — a_d = x [k][lda], w_d = dy [k][ldw], both bf16 with k = B*T rows:
 * c[m][n] (=|+=) sum_kk a[kk][m] * w[kk][n]  (m, n multiples of 128, k of 64; a 128 x 128 split-K plan must exist: lmrl_gemm_bf16_splitk_ws_bytes).
 * No transposed copy of x or dy is needed (the kernel gathers MFMA operands with ds_read_b64_tr_b16). */
int lmrl_gemm_bf16_splitk_kmajor(const void *a_d, const void *w_d, void *c_d, int m, int n, int k, int lda, int ldw, int ldc, int n_store, int accumulate,
                                 void *ws_d, void *stream);
/* colsum_d[c] (=|+=) sum_r src[r][c] of a staged bf16 matrix [rows][ld_src] — a Dense layer's bias gradient from its staged dy; ws_d: at least
 * ceil(rows / 64) * cols floats.  Deterministic (fixed partition and order). */
int lmrl_colsum_bf16(const void *src_d, long ld_src, int rows, int cols, float *colsum_d, int accumulate, float *ws_d, void *stream);

/* TOOLS ONLY (tools/bench_gemm.py tile-configuration sweeps; never called by the package): forces a GEMM tile configuration,
 * 0 = the shape policy, 1 = the round-1 register-staged kernels, 10.. = fixed tiles. */
void lmrl_gemm_set_variant(int v);

/* ------------------------------------------------------------------------------------------
 * Fused LM-head + sampling (csrc/sampler.hip).  Replaces logits[:, -1] -> warpers -> jax.random.categorical in
 * the reference's generation loop and the ILQL perturbation logits = pi_beta + beta*min(q1,q2)
 * (LLM_RL/algorithms/value_rl_base/gpt2/generation.py:97-119).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    float temperature;      /* <= 0: greedy (do_sample=False) */
    int32_t top_k;          /* <= 0: off; needs logits_out_d (1 .. 64 on the Philox path — policy-only and ILQL value-policy heads alike: scratch of
                             * the rare rows the fused candidate selection hands back, NOT the logits, unless `flags` asks for them; otherwise
                             * the logits are materialised there) */
    uint64_t seed;          /* Philox key */
    uint32_t step;          /* counter word: one per sampled token position */
    float steer_strength;   /* added to logit[steer_tok_d[row]] (synthetic workloads only; 0 = off) */
    float beta;             /* ILQL logit perturbation weight */
    int32_t pad_token;      /* written for inactive rows */
    const uint32_t *epoch_d;/* optional DEVICE word = 4th Philox counter word (0 when NULL): fresh noise per hipGraph replay */
    float top_p;            /* nucleus mass in (0, 1); <= 0 or >= 1 = off.  Applied after temperature and top_k (HF warper order):
                             * the smallest prefix of the descending-sorted tokens whose cumulative probability reaches top_p */
    int32_t rng;            /* LMRL_RNG_PHILOX (0, default): the package's own counter stream above.
                             * LMRL_RNG_JAX: the stream of `jax.random.categorical(key, logits[m, vocab])` as HF-Flax `_sample` calls it for the
                             * reference (ppo/gpt2/interface.py:524-535): `seed` = the call's PRNG key, (key[0] << 32) | key[1]; Gumbel word of
                             * (row, column) = element row * vocab + column of jax.random.gumbel(key, (m * vocab,)) — threefry2x32-20 over the
                             * iota split in halves (csrc/threefry.h); logits / temperature by division; `step` and `epoch_d` are unused (the
                             * caller walks the key schedule: lmrl_gym_amd/jax_prng.py).  All m rows of the call form ONE noise array. */
    int32_t flags;          /* LMRL_SAMPLE_WANT_LOGITS: the caller reads logits_out_d after the call — materialise them even where the fused top-k
                             * path would not (same tokens either way) */
} lmrl_sample_params;
#define LMRL_SAMPLE_WANT_LOGITS 1
#define LMRL_SAMPLE_KEEP_PARTIALS 2 /* lmrl_lm_head_sample: leave the per-(row, tile) partials in ws_d and do NOT launch the reduce — the caller merges them
                                     * (lmrl_wordle_sample_accept_embed); token_d / logprob_d are not written, but logprob_d (null or not) still selects whether
                                     * the partials carry the log-sum-exp pieces: pass the SAME logprob_d, null or not, to both calls — a log-prob merged from
                                     * partials made with logprob_d = NULL is garbage.  Policy-only Philox or greedy sampling without
                                     * top_k / top_p only (LMRL_ERR_ARG otherwise: no other path leaves those partials) */
#define LMRL_RNG_PHILOX 0
#define LMRL_RNG_JAX 1
/* host faces of the LMRL_RNG_JAX stream: the Threefry-2x32 (20 rounds) block function and words [i0, i0 + count) of
 * jax.random.bits(key, (n,), uint32) — for known-answer tests without a GPU */
void lmrl_threefry2x32(const uint32_t key[2], const uint32_t ctr[2], uint32_t out[2]);
int lmrl_jax_random_bits_host(const uint32_t key[2], uint32_t n, uint32_t i0, uint32_t count, uint32_t *out);

/* workspace of lmrl_lm_head_sample (per-(row, tile) partials or top-k candidate records + the flagged-row list).  One workspace per concurrent stream. */
size_t lmrl_sample_ws_bytes(int m, int vocab_padded);
/* byte offset, inside that workspace, of the fused top-k path's flagged-row list: int32 words — [0] = rows the exactness check handed back to the
 * materialised path in the LAST call (diagnostics / tests), 15 reserved words, 64 per-row-block flags, then the row indices */
size_t lmrl_sample_fb_offset(int m, int vocab_padded);
/* hidden_d bf16 [m][d] . wte_d bf16 [vocab_padded][d]^T -> token_d[m] (+ logprob_d[m] under the sampling
 * distribution).  Optional ILQL operands: q_hidden{1,2}_d bf16 [m][d] (= relu(dense1(h)) of each Q head),
 * q_w{1,2}_d bf16 [vocab_padded][d] (dense2 kernels, [out][in]), q_b{1,2}_d f32 [vocab_padded].
 * logits_out_d (optional f32 [m][vocab_padded]) receives the combined (untempered) logits — except on the fused warper path
 * (either random stream, one to three operands, temperature > 0, and 0 < top_k <= 256 [above 64: top_k <= vocab_padded / 128] and / or
 * 0 < top_p < 1: `FlaxTopKLogitsWarper` / `FlaxTopPLogitsWarper` of train_ppo_gpt2.py:98-99, 218-227 inside the LM-head epilogue): there the
 * epilogue keeps the 8 largest logits of every (row, 128-column tile) — and, for top_p without top_k, the tile's probability mass —, a reduce
 * kernel finds the row's k-th largest among them / the nucleus' crossing token, checks that no tile can hide a logit that matters, and draws;
 * logits_out_d is written only for the 128-row blocks of rows that fail the check (they are re-done from materialised logits: same tokens as
 * the materialised path in every case).  LMRL_SAMPLE_WANT_LOGITS in p->flags: always materialise. */
int lmrl_lm_head_sample(const void *hidden_d, const void *wte_d, const void *q_hidden1_d, const void *q_w1_d,
                        const float *q_b1_d, const void *q_hidden2_d, const void *q_w2_d, const float *q_b2_d, int m,
                        int d_model, int vocab, int vocab_padded, const lmrl_sample_params *p, const int32_t *steer_tok_d,
                        const uint8_t *active_d, int32_t *token_d, float *logprob_d, float *logits_out_d, void *ws_d,
                        void *stream);
/* Generation bookkeeping for any tokenizer (the per-token host loop of HF `generate` / GPT2PPOPolicy.act, ppo/gpt2/interface.py:
 * 527-535): for every live row append sampled_d[row] to out_tokens_d[row][out_len_d[row]++]; a row stops (active_d[row] = 0) at
 * eos_token (< 0: none) or at `cap` tokens; next_tok_d / next_cnt_d are the inputs of the next single-token forward. */
int lmrl_gen_accept(const int32_t *sampled_d, uint8_t *active_d, int32_t *out_tokens_d /* [n][cap] */, int32_t *out_len_d,
                    int32_t *next_tok_d, int32_t *next_cnt_d, int eos_token, int cap, int n, void *stream);
/* Sample from materialised logits (temperature, top-k, top-p) with the same random stream. */
int lmrl_sample_logits(const float *logits_d, int ld, int m, int vocab, const lmrl_sample_params *p,
                       const uint8_t *active_d, int32_t *token_d, float *logprob_d, void *stream);
/* the same, after adding p->steer_strength to logits_d[row][steer_tok_d[row]] IN PLACE (synthetic workloads; the fused path does this in
 * its epilogue) — the sampling step of the fp32 rollout mode, whose LM head is a plain fp32 GEMM */
int lmrl_sample_logits_steer(float *logits_d, int ld, int m, int vocab, const lmrl_sample_params *p, const int32_t *steer_tok_d,
                             const uint8_t *active_d, int32_t *token_d, float *logprob_d, void *stream);

/* ------------------------------------------------------------------------------------------
 * fp32 rollout mode (csrc/attn_cached_f32.hip + the fp32 train-step kernels below): the reference's DEFAULT rollout arithmetic is float32
 * (llm_rl_scripts/wordle/bc/eval_bc_gpt2.py:34,69); `lmrl_gym_amd.gpt2_f32_engine.GPT2EngineF32` sequences these calls — lmrl_embed_fwd,
 * lmrl_layernorm_fwd, lmrl_sgemm (exact fp32 MFMA), lmrl_gelu_fwd — around an fp32 K/V cache.
 * Its value policies (ILQL / MC) take their LM head from lmrl_value_head_logits_f32 (below, with lmrl_sgemm) in "f32" mode and from
 * lmrl_lm_head_sample on three split operands in "bf16x3" mode.
 *   lmrl_chunk_begin_f32  pos[b*c + j] = len[b] + j for j < cnt[b]; padding slots get position 0 and token id 0
 *   lmrl_attn_cached_f32  one layer's attention for the c new tokens of every env: qkv_d fp32 [b*c][3*H*64]; kcache_d / vcache_d fp32
 *                         [b][tmax][H*64]; query j sees the cached positions [0, len[b]) and the chunk's tokens [0, j]; appends the new
 *                         K / V rows at len[b] + j; out_d fp32 [b*c][H*64] (padding slots untouched).  c == 1 (single-token decode) runs the
 *                         batched-load kernel (one wave per (env, head), 32 cached positions requested before any arithmetic).
 *   lmrl_attn_cached_f32_split3  the same, and (split3_out_d != NULL) the output ALSO as the bf16 three-term split operand
 *                         [b*c][3*H*64] = [hi | lo | hi] of the projection GEMM of the bf16x3 mode (lmrl_split3_bf16's layout and rounding)
 *   lmrl_chunk_end_f32    last_d[b] = x_d[b*c + cnt[b] - 1] (envs with cnt == 0 keep theirs), then len[b] += cnt[b]
 * ------------------------------------------------------------------------------------------ */
int lmrl_chunk_begin_f32(const int32_t *len_d, const int32_t *cnt_d, int32_t *ids_d, int32_t *pos_d, int b, int c, int n_pos, void *stream);
int lmrl_attn_cached_f32(const float *qkv_d, float *kcache_d, float *vcache_d, const int32_t *len_d, const int32_t *cnt_d, float *out_d, int b, int c,
                         int n_head, int tmax, void *stream);
int lmrl_attn_cached_f32_split3(const float *qkv_d, float *kcache_d, float *vcache_d, const int32_t *len_d, const int32_t *cnt_d, float *out_d,
                                void *split3_out_d, int b, int c, int n_head, int tmax, void *stream);
int lmrl_chunk_end_f32(const float *x_d, const int32_t *cnt_d, float *last_d, int32_t *len_d, int b, int c, int d, void *stream);

/*
 * fp32 prompt-prefix cache (csrc/kv_prefix_f32.hip, csrc/attn_cached_f32.hip): the fp32 twins of lmrl_gpt2_kv_gather / lmrl_gpt2_kv_attach /
 * lmrl_gpt2_forward_prefixed for GPT2EngineF32 sessions (cache fp32 [n_layer][K|V][b][tmax][d]; last hidden and last residual fp32 [b][d]).
 *   lmrl_kv_gather_f32   env i of dst starts from row idx_d[i] of the prefix session src: K/V positions [0, n) of every layer with
 *                        n = min(src_len_d[row], dst_tmax, src_tmax), dst_len_d[i] = n and (optional) the row's last hidden state and last
 *                        residual.  idx_d[i] < 0 (or >= src_b): empty cache.  All layers in one launch; dst rows >= n are not written.
 *   lmrl_kv_attach_f32   the copy-free form: dst_len_d[i] = pfx_n_d[i] = n and the two last-state rows, nothing else; order_d (optional, [b]):
 *                        the envs grouped by prefix row (the launch order of the prefixed attention).
 *   lmrl_attn_decode_prefixed_f32  one layer's single-token decode attention (lmrl_attn_cached_f32_split3 with c = 1) for attached envs:
 *                        positions [0, n_d[i]) of env i are READ from row row_d[i] of the prefix session's layer cache pfx_k_d / pfx_v_d
 *                        ([pfx_rows][pfx_tmax][H*64]), positions [n_d[i], len_d[i]) from env i's own cache, and the new K / V row is
 *                        appended to env i's own cache at len_d[i].  order_d (optional): launch order, each XCD walking a contiguous stretch
 *                        of it.  Results are bit-identical to lmrl_attn_cached_f32_split3 after lmrl_kv_gather_f32 (same rows, same order
 *                        of arithmetic), split3_out_d included.
 */
int lmrl_kv_gather_f32(const float *src_kv_d, int src_b, int src_tmax, const int32_t *src_len_d, const float *src_hidden_d, const float *src_last_x_d,
                       const int32_t *idx_d, float *dst_kv_d, int dst_tmax, int b, float *dst_hidden_d, float *dst_last_x_d, int32_t *dst_len_d,
                       int n_layer, int d, void *stream);
int lmrl_kv_attach_f32(int src_b, int src_tmax, const int32_t *src_len_d, const float *src_hidden_d, const float *src_last_x_d, const int32_t *idx_d,
                       int b, int dst_tmax, float *dst_hidden_d, float *dst_last_x_d, int32_t *dst_len_d, int32_t *pfx_n_d, int32_t *order_d, int d,
                       void *stream);
int lmrl_attn_decode_prefixed_f32(const float *qkv_d, float *kcache_d, float *vcache_d, const int32_t *len_d, const int32_t *cnt_d, float *out_d,
                                  void *split3_out_d, int b, int n_head, int tmax, const float *pfx_k_d, const float *pfx_v_d, int pfx_rows,
                                  int pfx_tmax, const int32_t *row_d, const int32_t *n_d, const int32_t *order_d, void *stream);

/* ------------------------------------------------------------------------------------------
 * On-device token <-> game bookkeeping for lock-step Wordle rollouts (csrc/wordle_tokens.hip).
 * Replaces the per-turn host work of interact_environment + GPT2PPOPolicy.act
 * (LLM_RL/environment.py:180-206, LLM_RL/algorithms/ppo/gpt2/interface.py:519-546) and the text
 * (de)formatting of llm_rl_scripts/wordle/env/env.py:7-26.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t newline;          /* id of '\n' (= eos of an action, train_ilql_gpt2.py:393) */
    int32_t pad;
    int32_t letter_first[26]; /* 'a'..'z' as the first symbol of a line (no leading space) */
    int32_t letter_sp[26];    /* ' a'..' z' */
    int32_t sym_first[3];     /* 'g','y','b' */
    int32_t sym_sp[3];        /* ' g',' y',' b' */
    int32_t header[8];        /* ids of "Wordle:\n" (env.py:8) */
    int32_t n_header;
} lmrl_wordle_tokens;

/* Per-env rollout record, all device pointers owned by the caller; N envs, cap = traj_cap, G = max_new_tokens.
 * tokens/is_action/reward are exactly the fields of TokenTrajectory (LLM_RL/environment.py:329-380). */
typedef struct {
    int32_t *tokens;      /* [N][cap] */
    uint8_t *is_action;   /* [N][cap] */
    float *reward;        /* [N][cap]  reward on the last token of each action Text */
    int32_t *n_tok;       /* [N] */
    int32_t *gen;         /* [N][G] ids sampled for the current action */
    int32_t *gen_len;     /* [N] */
    uint8_t *gen_active;  /* [N] still generating the current action */
    uint8_t *env_done;    /* [N] episode finished */
    uint8_t *pend_newline;/* [N] action ended without eos: '\n' forced (interface.py:541) */
    int32_t *n_steps;     /* [N] env steps taken */
    float *ep_reward;     /* [N] sum of rewards */
} lmrl_wordle_traj;

typedef struct lmrl_wordle_tok_ctx lmrl_wordle_tok_ctx;
/* token_class (host, [vocab]): bits 0-24 up to five 5-bit letters, bits 25-27 their count (7 = any char other than
 * a-z / whitespace, or more than 5 letters, or whitespace between letters), bit 28 non-' ' whitespace before the first
 * letter (anywhere when the token has no letters), bit 29 non-' ' whitespace after the last letter. */
lmrl_wordle_tok_ctx *lmrl_wordle_tok_create(const lmrl_wordle_tokens *tokens, const uint32_t *token_class, int vocab,
                                            int max_new_tokens, int traj_cap);
void lmrl_wordle_tok_destroy(lmrl_wordle_tok_ctx *c);
/* episode start: trajectory := header tokens; first model chunk (chunk_tok_d [N][8], chunk_cnt_d [N]) := header */
int lmrl_wordle_tok_begin(lmrl_wordle_tok_ctx *c, const lmrl_wordle_traj *tr, int32_t *chunk_tok_d, int32_t *chunk_cnt_d,
                          int n, void *stream);
/* k-th sampled token of the current action: record it; envs that hit eos / max_new_tokens stop generating;
 * next_tok_d/next_cnt_d (and active_d) describe the next single-token decode step. */
int lmrl_wordle_tok_accept(lmrl_wordle_tok_ctx *c, const lmrl_wordle_traj *tr, const int32_t *sampled_d, int k,
                           int32_t *next_tok_d, int32_t *next_cnt_d, uint8_t *active_d, int n, void *stream);
/* One launch for what lies between two LM heads of the lock-step loop: the merge of lmrl_lm_head_sample's partials (called with
 * LMRL_SAMPLE_KEEP_PARTIALS; sample_ws_d is its workspace, active_d / token_d / logprob_d / pad_token its arguments), lmrl_wordle_tok_accept(k) on
 * the merged token, and — with m, ws_d (the c = 1 workspace of n envs) and len_d (the session's cache lengths) — the row embeddings of the
 * single-token forward over (next_tok_d, next_cnt_d) that follows, which is then called with LMRL_FWD_PRE_EMBEDDED.  m = ws_d = len_d = NULL:
 * no embedding (the action's last token).  One wave per env runs the three kernels' own bodies in their order: every output is bit-identical to
 * the three launches.  The model must run on the LN-folded path (LMRL_ERR_ARG otherwise). */
int lmrl_wordle_sample_accept_embed(lmrl_wordle_tok_ctx *c, const lmrl_wordle_traj *tr, const void *sample_ws_d, int vocab_padded, int pad_token,
                                    const uint8_t *active_d, int32_t *token_d, float *logprob_d, int k, int32_t *next_tok_d, int32_t *next_cnt_d,
                                    uint8_t *active_out_d, const lmrl_gpt2 *m, void *ws_d, const int32_t *len_d, int n, void *stream);
/* action tokens -> packed guess for lmrl_wordle_step (+ active mask = episode not done); appends the action to the record */
int lmrl_wordle_tok_guess(lmrl_wordle_tok_ctx *c, const lmrl_wordle_traj *tr, uint32_t *guess_d, uint8_t *active_d, int n,
                          void *stream);
/* env outputs -> reward placement, observation tokens, done flags, and the next model chunk
 * ([last unforwarded action token][forced '\n'] + observation tokens; count 0 for finished envs) */
int lmrl_wordle_tok_observe(lmrl_wordle_tok_ctx *c, const lmrl_wordle_traj *tr, const uint32_t *obs_d, const float *reward_d,
                            const uint8_t *flags_d, int32_t *chunk_tok_d, int32_t *chunk_cnt_d, int n, void *stream);
/* synthetic workloads: token spelling letter k (k = 5: '\n') of a scripted packed guess, for lmrl_sample_params.steer;
 * k < 0 writes all six positions at once, steer_d = int32 [6][n] */
int lmrl_wordle_tok_steer(lmrl_wordle_tok_ctx *c, const uint32_t *scripted_guess_d, int k, int32_t *steer_d, int n,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Rollout records -> the blocked ILQL / MC / BC datasets without leaving the device (csrc/offline_data.hip, csrc/offline_data_core.h).
 * Replaces the jsonl round trip of the offline trainers: data_gen.py:53-62 -> train_ilql_gpt2.py:123-152 (re-tokenisation,
 * ILQLData / MCData.from_token_trajectory_chain, ilql/data.py:18-79, mc_returns/data.py:21-74, block_sequences) and the
 * (ids, training mask) pairs of the BC scripts.
 * ------------------------------------------------------------------------------------------ */
/* The first n episodes of lmrl_wordle_policy_episodes' records (guess / obs / reward / flags [6][stride], n_turns [stride]) as lmrl_ppo_records
 * rows of pitch cap: the canonical ids of the REFORMATTED history ('Wordle:\n', 'a b c d e\n', 'g y b b y\n' or '\n'; env.py:7-17), is_action per
 * text, a turn's reward on the '\n' that closes its action, 0 on the header and the observations (TokenTrajectory.from_text_trajectory,
 * environment.py:349-380); slots past an episode's last token hold pad / 0 / 0.  done_d[e] = bit 0 of the last played turn's flags.
 * cap >= n_header + 72 holds every episode.  err_d (optional, one int32): episodes whose policy ran out of words (flag bit 3) or that do not
 * fit cap.  One wave per episode, lanes over token slots. */
int lmrl_wordle_tok_scripted_records(const lmrl_wordle_tokens *tokens, const uint32_t *guess_d, const uint32_t *obs_d, const float *reward_d,
                                     const uint8_t *flags_d, const int32_t *n_turns_d, int stride, int n, int cap, int32_t *tokens_d,
                                     uint8_t *is_action_d, float *rec_reward_d, int32_t *n_tok_d, uint8_t *done_d, int32_t *err_d, void *stream);
/* The same rule on ONE episode in host memory (guess6 / obs6 / reward6 / flags6: its six turns; CPU-tier tests, no GPU needed): fills
 * tokens_out / is_action_out / reward_out [cap], *done_out, returns the number of tokens (-1: bad argument, or the episode does not fit cap). */
int lmrl_wordle_host_scripted_record(const lmrl_wordle_tokens *tokens, const uint32_t *guess6, const uint32_t *obs6, const float *reward6,
                                     const uint8_t *flags6, int n_turns, int cap, int32_t *tokens_out, uint8_t *is_action_out, float *reward_out,
                                     int *done_out);
/* Outputs of lmrl_offline_block for m rows of width T = max_len; NULL = not wanted (input_ids and lengths are required). */
typedef struct {
    int32_t *input_ids;          /* [m][T]      tokens, padded with the pad id */
    uint8_t *should_take_action; /* [m][T - 1]  is_action[1:] */
    float *rewards;              /* [m][T - 1]  reward[1:] */
    float *returns;              /* [m][T - 1]  returns_d rows (MC reward-to-go already scattered to positions), blocked like rewards */
    float *training_mask;        /* [m][T]      float(is_action) per token: the segment weights of MaskDataset */
    uint8_t *dones;              /* [m]         the trajectory's own done: the chain's done on its last trajectory, 0 before */
    int32_t *lengths;            /* [m]         min(n_tok, T) */
    int32_t *next_token_ids;     /* [m][T]      multi-trajectory chains: the next trajectory's tokens up to (excluding) its first action at
                                                index >= 1, or all of it when it has none (ilql/data.py:62-71) */
    uint8_t *next_dones;         /* [m]         0 in the first case, the next trajectory's done in the second */
    int32_t *next_lengths;       /* [m] */
} lmrl_offline_blocks;
/* block_sequences(Padding.RIGHT, Truncation.RIGHT | LEFT (truncate_left != 0), max_len) of the rows keep_d[0 .. n_keep) of the records (keep_d NULL:
 * all n rows).  The [T - 1] arrays are x[1:] blocked with max_len - 1 ON THEIR OWN, as ILQLData.block / MCData.block do.  returns_d
 * [n][returns_pitch]: per source row the un-truncated reward-to-go on the shifted grid (lmrl_rtg over reward[1:] / is_action[1:]), required with
 * out->returns.  A chain's last trajectory has no next trajectory (None in the reference): its next_token_ids row is all padding, next_dones 1. */
int lmrl_offline_block(const lmrl_ppo_records *rec, const int32_t *keep_d, int n_keep, int max_len, int pad, int truncate_left, const float *returns_d,
                       int returns_pitch, const lmrl_offline_blocks *out, void *stream);
/* returns_d [n_chains] = the undiscounted sum of every reward of a chain (the score of bc/data.py:32-47's filter): summed in double in a fixed
 * order, rounded to float32 once.  The trajectories of a chain are consecutive rows. */
int lmrl_record_returns(const lmrl_ppo_records *rec, float *returns_d, void *stream);

/* ------------------------------------------------------------------------------------------
 * On-device token <-> game bookkeeping for lock-step Maze rollouts (csrc/maze_tokens.hip), for histories of one item
 * (last_k = 1, the reference's Maze harness: maze/bc/fully_observed_bc.py:230-237): a turn's prompt is the observation of the current
 * cell, a pure function of (goal, cell) (maze/env/env.py:8-81), so prompts come from a token table instead of the host tokenizer, and the
 * generated ids are decoded through a per-token byte table and matched against the four action strings (env.py:94-99) on the device.
 * Replaces the per-turn host work of interact_environment + GPT2PPOPolicy.act (LLM_RL/environment.py:180-206,
 * ppo/gpt2/interface.py:519-546).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t *pos;         /* [N][T]  (row << 16 | col) the turn's observation was rendered from */
    int32_t *gen;         /* [N][T][G] generated ids of the turn's action (before decoding) */
    int32_t *gen_len;     /* [N][T] */
    uint8_t *action;      /* [N][T]  LMRL_MAZE_LEFT..LMRL_MAZE_OTHER the decoded text maps to */
    float *reward;        /* [N][T] */
    uint8_t *kind;        /* [N][T]  LMRL_MAZE_KIND_* of the step's result */
    int32_t *n_turns;     /* [N] env steps taken */
    uint8_t *live;        /* [N] episode still running */
    float *ep_reward;     /* [N] */
    int32_t *obs_idx;     /* [N] row of the observation table for the current turn (-1: finished) */
    int32_t *out_tok;     /* [N][G] generation buffer of the current turn (lmrl_gen_accept) */
    int32_t *out_len;     /* [N] */
    uint8_t *gen_active;  /* [N] */
    uint8_t *act;         /* [N] action code of the current turn (input of lmrl_maze_step) */
    uint8_t *stepping;    /* [N] env takes part in the current turn (active mask of lmrl_maze_step) */
} lmrl_maze_traj;

typedef struct lmrl_maze_tok_ctx lmrl_maze_tok_ctx;
/* obs_tok [n_obs][obs_cap] / obs_len [n_obs]: token ids of every observation text, row = goal_slot * rows * cols + r * cols + c;
 * goal_slot [rows * cols]: slot of a goal cell (-1: not a goal of this table).  tok_bytes [vocab][16] / tok_blen [vocab]: the decoded
 * bytes of each token id; blen 0 = skipped (special tokens under skip_special_tokens=True, value_rl_base/base_interface.py:126),
 * 255 = not representable (non-ASCII or longer than 16 bytes: such a token cannot be part of an action string).  T = max_turns. */
lmrl_maze_tok_ctx *lmrl_maze_tok_create(const int32_t *obs_tok, const int32_t *obs_len, int n_obs, int obs_cap, const int32_t *goal_slot,
                                        int rows, int cols, const uint8_t *tok_bytes, const uint8_t *tok_blen, int vocab,
                                        int max_new_tokens, int max_turns);
void lmrl_maze_tok_destroy(lmrl_maze_tok_ctx *c);
/* episode start (after lmrl_maze_reset): every env live, counters cleared */
int lmrl_maze_tok_begin(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, int n, void *stream);
/* turn start: obs_idx from the env state (pos, goal), position recorded, generation buffers cleared, gen_active = live */
int lmrl_maze_tok_turn(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, const void *state_d, int n, void *stream);
/* chunk j (chunk tokens per env) of the current prompts for a prefill forward: chunk_tok_d [N][chunk], chunk_cnt_d [N] */
int lmrl_maze_tok_prompt(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, int j, int chunk, int32_t *chunk_tok_d, int32_t *chunk_cnt_d,
                         int n, void *stream);
/* generated ids -> action code: text = concat(token bytes, special tokens skipped); `text.removesuffix('\n') + '\n'`
 * (the Maze scripts' out_str_process) compared with the four action strings; records ids and code */
int lmrl_maze_tok_action(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, int n, void *stream);
/* The finished episodes as PPO records (lmrl_ppo_records): one token trajectory per transition — observation ids ++ action ids, the step reward on the
 * action's last token.  Action ids: a legal action (its post-processed text is a key of the action dict) as the tokenizer's encoding of that key when
 * lmrl_maze_tok_set_actions was called; otherwise the generated ids minus special tokens (byte_ids != 0 — a tokenizer whose ids are the text's UTF-8
 * bytes: the bytes of every decoded token), + newline_tok when the decoded text does not end in a newline.  Chained per episode,
 * as the online scripts build them (llm_rl_scripts/maze/ppo/train_ppo_online.py:444-465 + LLM_RL/environment.py:359-370).  off_d [n + 1] =
 * exclusive scan of tr->n_turns (lmrl_exclusive_scan_i32); rows off_d[e] + t; outputs [off_d[n]][cap] / [off_d[n]], done_d / chain_total_d [n]
 * (a chain's concatenated length: the GAE row pitch is their maximum).  The first n of the engine's n_envs envs are exported. */
int lmrl_maze_tok_ppo_records(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, const void *state_d, int n, int n_envs, const int32_t *off_d, int newline_tok,
                              int byte_ids, int cap, int32_t *tokens_d, uint8_t *is_action_d, float *reward_d, int32_t *n_tok_d, int32_t *chain_d, int32_t *pos_d, uint8_t *last_d,
                              uint8_t *done_d, int32_t *chain_total_d, void *stream);
/* The same export for item windows (last_k > 1; run after an episode of the history-mode loop below), in the form of the partially observed online
 * script (llm_rl_scripts/maze/ppo/partially_observed_ppo_online.py:372-398): per transition ONE non-action text — the window's item texts joined by
 * single spaces — then the action text, reward on the action's last token; chained per episode.  The window of every turn is rebuilt from the record
 * (tr->pos / action / kind: maze/env/env.py:179-184).  Token ids: the first item's own encoding, every later item's encoding behind the joining space
 * (lmrl_maze_tok_set_spaced), a legal action as the encoding of its dict key (lmrl_maze_tok_set_actions), any other action string as its generated
 * ids (as above) — or, with byte_ids != 0 (a tokenizer whose ids are the text's UTF-8 bytes), as the bytes of its decoded text, i.e. exactly
 * tokenizer.encode(text) also when the policy spelled it with multi-byte tokens.  last_k <= 64.  tokens_d == NULL: first pass — only n_tok_d (untruncated lengths) .. chain_total_d are written, the caller sizes
 * `cap` by the longest row and calls again. */
int lmrl_maze_tok_ppo_records_hist(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, const void *state_d, int n, int n_envs, const int32_t *off_d, int last_k,
                                   int newline_tok, int byte_ids, int cap, int32_t *tokens_d, uint8_t *is_action_d, float *reward_d, int32_t *n_tok_d, int32_t *chain_d,
                                   int32_t *pos_d, uint8_t *last_d, uint8_t *done_d, int32_t *chain_total_d, void *stream);
/* host tables for the above: obs_sp_tok [n_obs][obs_sp_cap] / obs_sp_len [n_obs] = tokenizer.encode(' ' + observation text) of every row of the
 * observation table, act_sp_tok [4][act_sp_cap] = tokenizer.encode(' ' + action string), its length in the last slot */
int lmrl_maze_tok_set_spaced(lmrl_maze_tok_ctx *c, const int32_t *obs_sp_tok, const int32_t *obs_sp_len, int obs_sp_cap, const int32_t *act_sp_tok,
                             int act_sp_cap);
/* Histories of more than one item (MazeEnv(last_k > 1): `(history + [action] + [observation])[-last_k:]`, maze/env/env.py:182-184; the prompt is the
 * window's text, left-truncated to max_input_length tokens, ppo/gpt2/interface.py:519-524; partially_observed_bc.py:241 runs last_k = 40) on a
 * persistent per-env KV cache.  Per env: the episode's token history, the token offset of every item, and which part of the history is in the
 * cache.  "Append" turns (window still growing: prompt t + 1 = prompt t ++ action ++ observation token for token) forward only the action's
 * unforwarded tail + the new observation; "re-prefill" turns (window slid or truncated: every position shifts under GPT-2's absolute position
 * embeddings) forward the window again from position 0.  The caller schedules the kind per turn (`reprefill`) from static bounds and says how many
 * tokens per env the turn's chunk forwards cover (`feed_budget`); an env whose window moved in an append turn (e.g. restarted by an illegal action
 * string) is simply re-forwarded within that budget; flags[0] bit 0 = it did not fit, bit 1 = history buffer / item table overflow.  len0_d / len1_d: the cache-length arrays of the
 * policy's (and, optional, the value base's) KV session, kept in step by these calls. */
typedef struct {
    int32_t *hist;        /* [N][hcap] ids of every item of the episode, in order */
    int32_t *item_off;    /* [N][max_items + 1] token offset of item k (item_off[k + 1]: its end) */
    int32_t *n_items;     /* [N] */
    int32_t *feed_start;  /* [N] first history token that goes through the model this turn */
    int32_t *feed_len;    /* [N] */
    int32_t *cache_len;   /* [N] history tokens [base, base + cache_len) sit in the KV cache at positions [0, cache_len) */
    int32_t *base;        /* [N] */
    int32_t *prompt_len;  /* [N] tokens of the current prompt */
    int32_t *win_floor;   /* [N] first item of the window since the env last returned (observation,) alone (LMRL_MAZE_KIND_OBS_ONLY, env.py:179-180) */
    int32_t *flags;       /* [1] */
    int32_t hcap, max_items;
} lmrl_maze_hist;
int lmrl_maze_hist_begin(const lmrl_maze_hist *h, int32_t *len0_d, int32_t *len1_d, int n, void *stream);
/* after lmrl_maze_tok_turn: the current observation joins the history; window / truncation / feed range of every env */
int lmrl_maze_hist_observe(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, const lmrl_maze_hist *h, int last_k, int max_input_length, int reprefill,
                           int feed_budget, int32_t *len0_d, int32_t *len1_d, int n, void *stream);
/* chunk j of this turn's feed for a prefill forward: chunk_tok_d [N][chunk], chunk_cnt_d [N] */
int lmrl_maze_hist_chunk(const lmrl_maze_hist *h, int j, int chunk, int32_t *chunk_tok_d, int32_t *chunk_cnt_d, int n, void *stream);
/* act_tok (host) [4][act_cap]: the tokenizer's encoding of 'move left\n' / 'move right\n' / 'move up\n' / 'move down\n' (LMRL_MAZE_LEFT ..), the length of
 * each in its last slot — what a later prompt holds for a legal action, whatever ids the policy generated to spell it */
int lmrl_maze_tok_set_actions(lmrl_maze_tok_ctx *c, const int32_t *act_tok, int act_cap);
/* after lmrl_maze_tok_action: the action joins the history — a legal action as its encoding above, an illegal string (it never reaches a later
 * prompt: the env answers with the observation alone) as its generated ids; the cache is cut back to the prompt + the forwarded generated ids
 * that ARE the action's ids */
int lmrl_maze_hist_action(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, const lmrl_maze_hist *h, int32_t *len0_d, int32_t *len1_d, int n, void *stream);
/* outputs of lmrl_maze_step -> record (reward, kind), counters, live &= !done */
int lmrl_maze_tok_result(lmrl_maze_tok_ctx *c, const lmrl_maze_traj *tr, const float *reward_d, const uint8_t *done_d,
                         const uint8_t *kind_d, int n, void *stream);

/* ------------------------------------------------------------------------------------------
 * On-device token <-> game bookkeeping for lock-step chess rollouts (csrc/chess_tokens.hip) around the rules of csrc/chess_rules.h: the chess
 * twin of the Maze loop above for `FenChessHistoryEnv` (chess/env/env.py:213-238; the online PPO script chess/ppo/train_ppo_gpt2_online.py:201-340).
 * A turn's prompt is `' '.join(fen)` of the current position alone (preprocess_state_og): no history window, no prefix cache — only the K/V
 * rows of the prefix the prompt shares with the previous turn's are kept (lmrl_chess_tok_prefix).  Replaces the
 * per-turn host work of interact_environment + GPT2PPOPolicy.act + VectorChessEnv.step.  Every buffer is the caller's; all calls are asynchronous
 * on `stream`.  One game per lane.  N envs, T = max_turns, G = max_new_tokens; strings are fixed-pitch and NUL-padded as above.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    /* the episode record, one row per (env, turn) */
    char *fen;            /* [N][T][LMRL_CHESS_FEN_BYTES] position text the turn's prompt was rendered from (turn 0: the start position as given) */
    int32_t *gen;         /* [N][T][G] generated ids of the turn's action */
    int32_t *gen_len;     /* [N][T] */
    char *action;         /* [N][T][LMRL_CHESS_ACTION_BYTES] the SAN string handed to the board */
    uint8_t *result;      /* [N][T] LMRL_CHESS_ILLEGAL .. LMRL_CHESS_NULL_MOVE */
    float *reward;        /* [N][T] after the opponent's half (-1: the agent was mated) */
    uint8_t *done;        /* [N][T] game over, or more than max_moves agent moves made */
    char *opp_san;        /* [N][T][LMRL_CHESS_ACTION_BYTES] the opponent's reply in SAN ("" when there was none) */
    char *reply;          /* [N][T][8] the same reply in UCI form */
    int32_t *n_turns;     /* [N] env steps taken */
    uint8_t *live;        /* [N] episode still running */
    float *ep_reward;     /* [N] */
    /* the current turn */
    char *cur_fen;        /* [N][LMRL_CHESS_FEN_BYTES] the observation the next prompt is rendered from */
    int32_t *cur_len;     /* [N] its length */
    char *prev_fen;       /* [N][LMRL_CHESS_FEN_BYTES] the observation of the previous turn's prompt (its K/V rows are still in the cache) */
    int32_t *prev_len;    /* [N] its length (0: none) */
    int32_t *keep;        /* [N] prompt tokens of the current turn whose K/V rows are kept from the previous turn (lmrl_chess_tok_prefix) */
    int32_t *out_tok;     /* [N][G] generation buffer (lmrl_gen_accept) */
    int32_t *out_len;     /* [N] */
    uint8_t *gen_active;  /* [N] */
    char *act;            /* [N][LMRL_CHESS_ACTION_BYTES] the decoded action */
    uint8_t *res;         /* [N] result of the agent's half-step (255: env not stepping) */
    float *rew;           /* [N] */
    uint8_t *dn;          /* [N] */
    char *uci;            /* [N][8] the agent's move in UCI form where a reply is wanted (result MOVED), "" elsewhere: what goes DOWN to a host engine */
    char *cur_reply;      /* [N][8] the reply in UCI form: written by lmrl_chess_tok_opponent, or by the caller before lmrl_chess_tok_opponent_host */
    uint8_t *reply_ok;    /* [N] 0: the reply was not a legal move of the position */
    char *cur_san;        /* [N][LMRL_CHESS_ACTION_BYTES] */
    int32_t *flags;       /* [1] bit 0: a prompt was longer than the chunks scheduled for it (lmrl_chess_tok_prompt) */
} lmrl_chess_traj;

typedef struct lmrl_chess_tok_ctx lmrl_chess_tok_ctx;
/* byte_id (host, [256]): the id of every single-byte string (-1: none) — a prompt is `tokenizer.encode(' '.join(fen))` for tokenizers that encode
 * that text character by character (the caller probes it).  tok_bytes [vocab][16] / tok_blen [vocab]: as lmrl_maze_tok_create.  byte_ids != 0: ids
 * 0..255 ARE the text's UTF-8 bytes and every other id decodes to nothing (then a generation is decoded as UTF-8 with Python's errors="ignore").
 * eos_token < 0: none.  max_turns < 4096.  host_only != 0: no device tables — only the lmrl_chess_host_* faces below work (CPU tests). */
lmrl_chess_tok_ctx *lmrl_chess_tok_create(const int32_t *byte_id, const uint8_t *tok_bytes, const uint8_t *tok_blen, int vocab, int byte_ids, int eos_token,
                                          int max_new_tokens, int max_turns, int host_only);
void lmrl_chess_tok_destroy(lmrl_chess_tok_ctx *c);
/* episode start: chess.Board(fen) for every env from fens_d [n][LMRL_CHESS_FEN_BYTES] (ok_d[i] = 0: malformed, env not live), records cleared, the
 * start text becomes the first observation */
int lmrl_chess_tok_begin(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, void *pos_d, const char *fens_d, uint8_t *ok_d, int n, void *stream);
/* turn start: how much of the cache survives.  The caches still hold the previous turn's prompt at positions [0, its length); with reuse != 0 the
 * K/V rows of the longest common prefix of the previous and the current (left-truncated) prompt are kept, at least one token is forwarded again —
 * the rule of the generic policy's prefill (`GPT2PPOPolicy(reuse_kv=True)`): after an illegal move the position and so the prompt is unchanged
 * and one token goes through the model, after a move the rows up to the first changed square stay.  len_d [N]: the KV session's cache lengths,
 * set to keep[env] (0 with reuse == 0, on an episode's first turn, and for finished envs). */
int lmrl_chess_tok_prefix(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, int max_input_length, int reuse, int32_t *len_d, int n, void *stream);
/* chunk j of n_chunks (chunk tokens per env) of the part of the current prompts (left-truncated to max_input_length tokens) behind the kept prefix,
 * for a prefill forward: chunk_tok_d [N][chunk], chunk_cnt_d [N] (0 for finished envs).  A prompt that does not fit n_chunks * chunk tokens sets
 * flags bit 0. */
int lmrl_chess_tok_prompt(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, int j, int chunk, int max_input_length, int n_chunks, int32_t *chunk_tok_d,
                          int32_t *chunk_cnt_d, int n, void *stream);
/* generated ids (out_tok / out_len) -> the SAN string of the host path: ids up to the first eos -> text (special ids skipped) -> the policy's
 * `removesuffix('\n') + '\n'` -> postprocess_move (every ' ' removed, then str.strip()) -> non-ASCII characters as '?', at most
 * LMRL_CHESS_ACTION_BYTES - 1 bytes (VectorChessBoards._strings); then the agent's half of ChessEnv.step: res / rew / dn / uci */
int lmrl_chess_tok_action(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, void *pos_d, int n, void *stream);
/* the device opponent, for games whose result is LMRL_CHESS_MOVED: one of the position's legal moves (lmrl_chess_describe's order) is played.
 * reply_idx_d == NULL: the counter-based reply stream — legal_moves[(word * count) >> 32] with
 *     word = first output word of Philox4x32-7 (the sampler's function: csrc/sampler.hip, oracle/gpt2.py `philox4x32_10(..., rounds=7)`),
 *     counter = (env, turn of the env, LMRL_CHESS_REPLY_STREAM, *epoch_d [0 when NULL]), key = (seed low word, seed high word);
 * epoch_d is read on the device when the kernel runs, so a captured turn draws fresh replies on every replay (the caller advances it, as the
 * sampler's epoch).  A stream of this package's own: the reference draws from numpy's global state in env order (env.py:178).
 * reply_idx_d != NULL (int32 [reply_turns][n]): legal_moves[reply_idx[min(turn, reply_turns - 1)][env] mod count] (scripted workloads, tests). */
#define LMRL_CHESS_REPLY_STREAM 0x43484553u
int lmrl_chess_tok_opponent(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, void *pos_d, uint64_t seed, const uint32_t *epoch_d, const int32_t *reply_idx_d,
                            int reply_turns, int n, void *stream);
/* the host opponent (a UCI engine pool): the caller read tr->uci and wrote the replies into tr->cur_reply; reply_ok = 0 for an illegal one */
int lmrl_chess_tok_opponent_host(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, void *pos_d, int n, void *stream);
/* the turn into the record, the next observation (board.fen()), counters, live / gen_active for the next turn; done also once more than max_moves
 * agent moves were made (FenChessHistoryEnv) */
int lmrl_chess_tok_result(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, const void *pos_d, int max_moves, int n, void *stream);
/* The finished episodes of the first n envs as PPO records (lmrl_ppo_records), the twin of lmrl_maze_tok_ppo_records: one token trajectory per
 * transition — the (untruncated) prompt ids of the observation ++ the action ids, the reward on the action's last token — chained per episode as
 * chess/ppo/train_ppo_gpt2_online.py:293-314 builds them.  Action ids = the encoding of the action TEXT `decode(ids).removesuffix('\n') + '\n'`:
 * byte ids: the UTF-8 bytes of the decoded characters; otherwise the generated ids up to eos minus special ids; newline_tok appended when the text
 * does not end in a newline.  off_d [n + 1] = exclusive scan of tr->n_turns. */
int lmrl_chess_tok_ppo_records(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, int n, const int32_t *off_d, int newline_tok, int cap, int32_t *tokens_d,
                               uint8_t *is_action_d, float *reward_d, int32_t *n_tok_d, int32_t *chain_d, int32_t *pos_d, uint8_t *last_d, uint8_t *done_d,
                               int32_t *chain_total_d, void *stream);
/* host faces of the string work (the same functions on host memory; no GPU needed): the prompt ids of a position text (-> count, -1: out_cap too
 * small), the action bytes of a generation (out: LMRL_CHESS_ACTION_BYTES bytes, -> length), one word of the reply stream */
int lmrl_chess_host_prompt_tokens(const lmrl_chess_tok_ctx *c, const char *fen, int max_input_length, int32_t *out, int out_cap);
int lmrl_chess_host_action_from_tokens(const lmrl_chess_tok_ctx *c, const int32_t *ids, int n, char *out);
uint32_t lmrl_chess_host_reply_word(uint64_t seed, uint32_t epoch, uint32_t turn, uint32_t env);

/* ------------------------------------------------------------------------------------------
 * On-device token <-> game bookkeeping for lock-step Twenty Questions rollouts (csrc/tq_tokens.hip; the text rules: csrc/tq_core.h): the twin of
 * the loops above for `BatchedTwentyQuestionsPolicyEnvironment` + `GPT2EngineOracle` (twenty_questions/env/{env,data,oracle}.py; the PPO script
 * twenty_questions/ppo/train_ppo.py), the env with TWO models in the loop.  A turn: guesser decode | lmrl_tq_question | oracle prefill
 * (lmrl_tq_oracle_prompt per chunk) | <= oracle_max_new_tokens greedy steps | lmrl_tq_answer | lmrl_tq_judge | guesser chunks
 * (lmrl_tq_history_chunk).  Tokenizers whose ids are the text's UTF-8 bytes only (the caller probes it); histories that fit without truncation.
 * Every buffer is the caller's; all calls are asynchronous on `stream`.  One env per lane.  N envs, T = max_turns, G = max_new_tokens,
 * Q = G + 1 question bytes, OG = oracle_max_new_tokens.
 * ------------------------------------------------------------------------------------------ */
#define LMRL_TQ_ORACLE_MAX_NEW 16
typedef struct {
    /* the episode record, one row per (env, turn) */
    int32_t *gen;         /* [N][T][G] the guesser's generated ids */
    int32_t *gen_len;     /* [N][T] */
    uint8_t *q_text;      /* [N][T][Q] the question as the history holds it: decode(ids) under `removesuffix('\n') + '\n'` */
    int32_t *q_len;       /* [N][T] */
    int32_t *q_off;       /* [N][T] where the question's ids start in hist */
    int32_t *ogen;        /* [N][T][OG] the oracle's generated ids */
    int32_t *ogen_len;    /* [N][T] */
    uint8_t *answer;      /* [N][T] 1 "Yes." / 0 "No." */
    float *reward;        /* [N][T] -1, or 0 for the question that guessed the word */
    uint8_t *done;        /* [N][T] */
    uint8_t *flag;        /* [N][T] 1: affirmed, but not judged on the device (the host decides after the episode) */
    int32_t *n_turns;     /* [N] questions asked */
    uint8_t *live;        /* [N] */
    float *ep_reward;     /* [N] */
    int32_t *word;        /* [N] index of the hidden word */
    /* the current turn */
    int32_t *out_tok;     /* [N][G] the guesser's generation buffer (lmrl_gen_accept) */
    int32_t *out_len;     /* [N] */
    uint8_t *gen_active;  /* [N] */
    int32_t *o_out_tok;   /* [N][OG] the oracle's generation buffer */
    int32_t *o_out_len;   /* [N] */
    uint8_t *o_active;    /* [N] */
    int32_t *strip_b;     /* [N] str.strip() of the current question = bytes [strip_b, strip_e) of its q_text row */
    int32_t *strip_e;     /* [N] */
    uint8_t *ans;         /* [N] the current answer code */
    int32_t *hist;        /* [N][hcap] canonical ids of the whole history: INITIAL_STR, question 1, answer 1, ... */
    int32_t *hist_len;    /* [N] */
    int32_t *feed_start;  /* [N] the guesser's pending feed = hist[feed_start, feed_start + feed_len) */
    int32_t *feed_len;    /* [N] */
    int32_t *o_prompt;    /* [N][pcap] the current oracle prompt */
    int32_t *o_len;       /* [N] */
    int32_t *o_prev;      /* [N][pcap] the previous turn's oracle prompt (its K/V rows are still in the oracle's cache) */
    int32_t *o_prev_len;  /* [N] */
    int32_t *o_keep;      /* [N] tokens of the current oracle prompt whose K/V rows are kept */
    int32_t *flags;       /* [1] bit 0: an oracle prompt's new part outgrew its chunks; 1: history overflow; 2: oracle prompt overflow (pcap);
                             3: a guesser feed outgrew its chunks */
    int32_t hcap, pcap;
} lmrl_tq_traj;

/* host tables of lmrl_tq_create.  One string table (`bytes` / `str_off [n_strings + 1]`): the determiners, the function words and the generic
 * nouns of the stand-in tagger (n_det, n_func, n_generic strings, in this order; envs/twenty_questions.py is their home), then every spelling's
 * lower-cased token list as the active tagger produced it (`WordVariants.tokens`): spelling p = strings [spell_off[p], spell_off[p + 1]), word
 * w = spellings [word_off[w], word_off[w + 1]).  prefix [n_words][prefix_cap] / prefix_len: the caller's encoding of
 * "Answer the question about the object truthfully.\nobject: {word}\nquestion: "; suffix: of "\nanswer (yes or no): "; invalid_question: the
 * bytes of INVALID_QUESTION; initial: the ids of INITIAL_STR; yes / no: of "Yes.\n" / "No.\n".  tok_blen [vocab]: 0 = the id adds nothing to a
 * decoded text (lmrl_maze_tok_create).  eos tokens < 0: none. */
typedef struct {
    const uint8_t *bytes;
    const int32_t *str_off, *spell_off, *word_off;
    int32_t n_strings, n_spellings, n_words, n_det, n_func, n_generic;
    const uint8_t *tok_blen;
    int32_t vocab, eos_token, oracle_eos_token;
    const int32_t *prefix, *prefix_len;
    int32_t prefix_cap;
    const int32_t *suffix;
    int32_t suffix_len;
    const uint8_t *invalid_question;
    int32_t invalid_len;
    const int32_t *initial;
    int32_t initial_len;
    const int32_t *yes;
    int32_t yes_len;
    const int32_t *no;
    int32_t no_len;
    int32_t max_new_tokens, oracle_max_new_tokens, max_turns;
} lmrl_tq_tables;

typedef struct lmrl_tq_ctx lmrl_tq_ctx;
/* the context owns copies of the tables only.  host_only != 0: no device copies — only the lmrl_tq_host_* faces work (CPU tests). */
lmrl_tq_ctx *lmrl_tq_create(const lmrl_tq_tables *tables, int host_only);
void lmrl_tq_destroy(lmrl_tq_ctx *c);
/* episode start.  Hidden word of env i: seeds_d[i] % n_words where deterministic_d[i] (NULL: nowhere), else draws_d[i] — the first
 * _randbelow(n_words) of random.Random(seed), drawn by the caller with lmrl_mt_seed + lmrl_mt_randbelow.  Records and counters cleared, envs
 * >= n_live idle, history = INITIAL_STR and pending as the guesser's first feed, both sessions' cache lengths 0. */
int lmrl_tq_reset(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, const uint64_t *seeds_d, const uint8_t *deterministic_d, const uint32_t *draws_d, int n_live,
                  int32_t *guesser_len_d, int32_t *oracle_len_d, int n, void *stream);
/* after the guesser's decode steps: generated ids -> the question text (UTF-8, errors="ignore"; `removesuffix('\n') + '\n'`) -> its canonical ids
 * onto the history; Python str.strip() of it -> the oracle prompt prefix[word] ++ stripped question ++ suffix (finished envs: INVALID_QUESTION
 * about their own word).  guesser_len_d: cut back to history + the generated ids that were forwarded AND are the canonical ids
 * (keep_generated == 0: to the history alone); oracle_len_d: the longest common prefix of the previous and this prompt, at least one token
 * forwarded — the rule of `GPT2PPOPolicy(reuse_kv=True)`. */
int lmrl_tq_question(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int keep_generated, int32_t *guesser_len_d, int32_t *oracle_len_d, int n, void *stream);
/* chunk j of n_chunks (chunk tokens per env) of the oracle prompts behind their kept prefixes: chunk_tok_d [N][chunk], chunk_cnt_d [N] */
int lmrl_tq_oracle_prompt(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int j, int chunk, int n_chunks, int32_t *chunk_tok_d, int32_t *chunk_cnt_d, int n, void *stream);
/* the same for the guesser's pending feed: the question's unforwarded canonical ids and the answer's (episode start: INITIAL_STR) */
int lmrl_tq_history_chunk(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int j, int chunk, int n_chunks, int32_t *chunk_tok_d, int32_t *chunk_cnt_d, int n, void *stream);
/* the oracle's generated ids -> strip().lower() -> yes|no at the start -> "Yes." / "No." (no match: "No."; a question equal to INVALID_QUESTION:
 * "No." unread); scripted_d (int8 [N][script_turns], NULL: none; < 0: ask the model): the injected answer of turn min(t, script_turns - 1).  The
 * answer's ids join the history and the guesser's feed. */
int lmrl_tq_answer(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, const int8_t *scripted_d, int script_turns, int n, void *stream);
/* guessed (an affirmed question that names the word: `is_done` under rule_pos_tag, questions of code points < 0x80), reward, done (guessed, or
 * max_conversation_length questions asked), the record, live flags.  An affirmed question with a byte >= 0x80 — with device_judge == 0 every
 * affirmed question — is not guessed here: the game goes on and the turn is flagged. */
int lmrl_tq_judge(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int device_judge, int max_conversation_length, int n, void *stream);
/* the first n envs' episodes as single-trajectory PPO records (lmrl_ppo_records without chains): the whole history's ids, the questions' tokens as
 * actions, each turn's reward on its question's last token, done [n]   (twenty_questions/ppo/train_ppo.py:322-352) */
int lmrl_tq_ppo_records(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int n, int cap, int32_t *tokens_d, uint8_t *is_action_d, float *reward_d, int32_t *n_tok_d,
                        uint8_t *done_d, void *stream);
/* host faces of the text rules (the same functions on host memory; no GPU needed): the question (-> length; strip_range[2] = its strip()), the
 * oracle prompt ids, the answer code, is_done (*judgeable = 0: a byte >= 0x80, not decided), the word draw */
int lmrl_tq_host_question(const lmrl_tq_ctx *c, const int32_t *ids, int n, uint8_t *question_out, int cap, int32_t *strip_range);
int lmrl_tq_host_oracle_prompt(const lmrl_tq_ctx *c, int word, const uint8_t *question, int n, int32_t *out, int cap);
int lmrl_tq_host_answer(const lmrl_tq_ctx *c, const uint8_t *question, int qn, const int32_t *ids, int n);
int lmrl_tq_host_is_done(const lmrl_tq_ctx *c, int word, const uint8_t *question, int n, int *judgeable);
int lmrl_tq_host_draw_word(uint64_t seed, int deterministic, int n_words);

/* ------------------------------------------------------------------------------------------
 * Per-kernel-class timing with HIP events on the launch stream (used by bench.py for the live roofline figure).
 * mask bit t enables tag t; `work` accumulates the algorithmic flops (GEMM-class tags) or bytes (others) per launch.
 * ------------------------------------------------------------------------------------------ */
void lmrl_prof_enable(unsigned mask);
void lmrl_prof_reset(void);
int lmrl_prof_n_tags(void);
const char *lmrl_prof_tag_name(int tag);
int lmrl_prof_read(int tag, double *total_ms, double *total_work, long long *launches);

/* ------------------------------------------------------------------------------------------
 * fp32 train-step building blocks (csrc/sgemm_f32.hip, csrc/train_ops.hip, csrc/losses.hip).
 * Together they restate GPT2PPOTrain._step / GPT2ILQLTrain._step (LLM_RL/algorithms/ppo/gpt2/interface.py:72-211,
 * LLM_RL/algorithms/ilql/gpt2/interface.py:88-367) in float32, the reference's default parameter/activation dtype.
 * ------------------------------------------------------------------------------------------ */
/* C[b] = alpha*op(A[b]).op(B[b]) + beta*C[b] (+bias[n]); row-major; op(A) MxK (trans_a: stored KxM), op(B) KxN
 * (trans_b: stored NxK); batch index = outer*nb_inner + inner with separate element strides. Exact fp32 (MFMA f32).
 * Unbatched products with few output tiles and a long K split K across workgroups: the partial products go to the caller's
 * workspace ws_d and a fixed-order reduce adds them (deterministic).  lmrl_sgemm_ws_bytes(m, n, k, nb_outer * nb_inner) is
 * its size, 0 when the product does not split; a splitting call with a NULL or smaller workspace fails before it launches
 * anything.  A captured graph keeps ws_d, and calls in flight on different streams need workspaces of their own. */
size_t lmrl_sgemm_ws_bytes(int m, int n, int k, int batch);
int lmrl_sgemm(int trans_a, int trans_b, int m, int n, int k, float alpha, const float *a_d, int lda, long sa_outer,
               long sa_inner, const float *b_d, int ldb, long sb_outer, long sb_inner, float beta, float *c_d, int ldc,
               long sc_outer, long sc_inner, int nb_outer, int nb_inner, const float *bias_d, void *ws_d, size_t ws_bytes,
               void *stream);
/* The value policy's LM head in exact fp32 (csrc/value_head_f32.hip; value_rl_base/gpt2/generation.py:100-119), element by element:
 *   pi = h . wte^T    q_i = qh_i . w2_i^T + b2_i    logits = fmaf(beta, qh2 ? fminf(q1, q2) : q1, pi)
 * h_d, qh{1,2}_d fp32 [m][d]; wte_d, w2_{1,2}_d fp32 [vocab_padded][d] ([out][in]); b2_{1,2}_d fp32 [vocab_padded]; logits_d fp32 [m][ld].
 * qh2_d, w2_2_d, b2_2_d all NULL: the MC-returns policy (no Q2).  Each product is bit-equal to lmrl_sgemm of the same operands (+ bias);
 * only the combined logits are written.  d % 64 == 0, vocab_padded % 128 == 0, ld >= vocab_padded, any m > 0; h / wte / qh / w2 16-byte
 * aligned.  No workspace, no device state: deterministic and capturable. */
int lmrl_value_head_logits_f32(const float *h_d, const float *wte_d, const float *qh1_d, const float *w2_1_d, const float *b2_1_d,
                               const float *qh2_d, const float *w2_2_d, const float *b2_2_d, float beta, int m, int d, int vocab_padded,
                               float *logits_d, int ld, void *stream);
/* A/B hook: 0 = auto (128x128 tiles when m, n >= 128, split K as above), 1 = always the 64x64-tile kernel, never split
 * (lmrl_sgemm_ws_bytes follows the setting) */
void lmrl_sgemm_set_variant(int v);
/* TOOLS / TESTS ONLY: bit 0 = LayerNorm forward, bit 1 = fused LayerNorm backward on the strided 4-byte-access kernels (A/B of the 16-byte-access
 * register-row kernels) */
void lmrl_train_ops_set_variant(int v);
/* TOOLS / TESTS ONLY: 1 = top-k / top-p sampling on the strided-row warper kernel also where the register-row kernel applies (A/B, equality tests) */
void lmrl_sampler_set_variant(int v);
/* TOOLS / TESTS ONLY: 1 = lmrl_gae / lmrl_rtg on the round-1 LDS-compaction kernel and the scalar whitening kernels, 2 = the 64-lane register
 * kernel also for chains of <= 128 slots, 3 = one slot per lane in the 16-lane DPP-row kernel (A/B, cross-checks of the two-slots-per-lane form) */
void lmrl_rl_reduce_set_variant(int v);
/* TOOLS / TESTS ONLY: bit 0 = bf16 flash-attention forward, bit 1 = dQ, bit 2 = dK/dV on the round-3 kernels (A/B and equality tests of the
 * round-4 sweeps: 128 queries per workgroup, two query groups per wave, global_load_lds tile ring) */
void lmrl_flash_set_variant(int v);
/* x[r] = wte[ids[r]] + wpe[pos[r]].  vocab > 0: wte has `vocab` rows and an id outside [0, vocab) embeds as a ZERO row — the pad id of a tokenizer
 * whose `<|pad|>` is the first id after the model's vocabulary (train_ppo_gpt2.py:124-126; the reference resizes the embedding and forces those
 * logits to -inf, ppo/gpt2/interface.py:330, so that id is never sampled and only ever sits at masked positions). */
int lmrl_embed_fwd(const float *wte_d, const float *wpe_d, const int32_t *ids_d, const int32_t *pos_d, float *x_d, int rows, int d, int vocab,
                   void *stream);
/* dwte[ids[r]] += dx[r], dwpe[pos[r]] += dx[r] without atomics (one owner wave per distinct index, fixed order: bit-reproducible).
 * live_d (optional, uint8 [rows]): rows with flag 0 are skipped — the padded positions of a right-padded batch (attention_mask == 0), whose dx is
 * exactly zero and which would otherwise all pile onto the pad id's owner wave.  t_row > 0 (the T of a [B, T] batch): a row whose flag is 0
 * but whose NEXT position in the same sequence has flag 1 stays live (the PPO / BC losses read row t wherever attention_mask[t + 1] is set, so
 * with left padding or holes its dx is not zero); right-padded batches: exactly the flagged rows.  vocab > 0: ids outside [0, vocab) own no
 * wte row (lmrl_embed_fwd) and are skipped. */
int lmrl_embed_bwd(const float *dx_d, const int32_t *ids_d, const int32_t *pos_d, const uint8_t *live_d, float *dwte_d, float *dwpe_d, int rows, int d,
                   int vocab, int t_row, void *stream);
/* Row compaction for the vocabulary-wide heads of the train steps: the losses read the Q / policy logits only on rows whose mask is set
 * (should_take_action x attention mask: ilql/base_interface.py:22-119, ppo/base_interface.py:72-142), so a head runs on the gathered rows
 * dst[i] = src[idx[i]] and its input gradient goes back with dst[idx[i]] (=|+=) src[i].  idx_d holds DISTINCT rows (no atomics). */
int lmrl_gather_rows_f32(const float *src_d, const int32_t *idx_d, float *dst_d, int n, int d, void *stream);
int lmrl_scatter_rows_f32(const float *src_d, const int32_t *idx_d, float *dst_d, int n, int d, int accumulate, void *stream);
int lmrl_layernorm_fwd(const float *x_d, const float *g_d, const float *b_d, float *y_d, float *mean_d, float *rstd_d, int rows, int d,
                       float eps, void *stream);
/* LayerNorm / gelu forward that ALSO write the bf16 copy of their output (row pitch ldb elements) — the operand of the GEMM that consumes it in
 * the bf16-matmul train mode (saves the separate lmrl_cast_bf16 pass).  y_d may be NULL: only the bf16 copy is kept (it also serves, transposed,
 * as the operand of the layer's dW product). */
int lmrl_layernorm_fwd_staged(const float *x_d, const float *g_d, const float *b_d, float *y_d, float *mean_d, float *rstd_d, void *yb_d, long ldb,
                              int rows, int d, float eps, void *stream);
/* x[r] += resid[r] (resid_d NULL: no add) and then LayerNorm of the updated row, in one pass: y (fp32, optional) and / or yb (bf16 [rows][ldb], the
 * operand of the consuming GEMM), mean / rstd for the backward.  The residual adds of an HF GPT-2 block (x + attn(ln_1 x), x + mlp(ln_2 x)) folded
 * into the LayerNorm that follows each of them (ln_2, the next block's ln_1, ln_f): x_d is the projection's raw output on entry, the residual
 * stream on exit. */
int lmrl_layernorm_add_fwd(float *x_d, const float *resid_d, const float *g_d, const float *b_d, float *y_d, float *mean_d, float *rstd_d, void *yb_d,
                           long ldb, int rows, int d, float eps, void *stream);
/* the same with the output written only as the "bf16 x 3" operand [rows][3 d] = [hi | lo | hi] (lmrl_split3_bf16's row format) — LayerNorm + split in one
 * pass for GPT2EngineF32's bf16x3 matmul mode (d a multiple of 256, <= 1280); lmrl_gelu_split3: gelu_new + split likewise ([rows][3 cols]). */
int lmrl_layernorm_add_fwd_split3(float *x_d, const float *resid_d, const float *g_d, const float *b_d, float *mean_d, float *rstd_d, void *split_d,
                                  int rows, int d, float eps, void *stream);
int lmrl_gelu_split3(const float *x_d, int rows, int cols, void *split_d, void *stream);
int lmrl_gelu_fwd_staged(const float *x_d, float *y_d, void *yb_d, long ldb, int rows, int cols, void *stream);
/* dx (=|+=) LN backward; dy_xhat_d (optional [rows][d]) receives dy*xhat whose column sum is d gamma */
int lmrl_layernorm_bwd(const float *dy_d, const float *x_d, const float *g_d, const float *mean_d, const float *rstd_d, float *dx_d,
                       float *dy_xhat_d, int rows, int d, int accumulate_dx, void *stream);
/* LayerNorm backward with the gamma / beta gradients reduced in the same pass (row slabs -> per-slab partial rows -> fixed-order sum):
 * dx (+)= ..., dgamma (+)= sum_r dy*xhat, dbeta (+)= sum_r dy.  d_model in {128, 256, 768, 1024, 1280, 1600} (the per-lane column
 * registers are compile-time); other widths use lmrl_layernorm_bwd + lmrl_colsum. */
int lmrl_layernorm_bwd_fused_supported(int d);
size_t lmrl_layernorm_bwd_fused_ws_bytes(int rows, int d);
int lmrl_layernorm_bwd_fused(const float *dy_d, const float *x_d, const float *g_d, const float *mean_d, const float *rstd_d, float *dx_d,
                             float *dgamma_d, float *dbeta_d, int rows, int d, int accumulate_dx, int accumulate_dg, float *ws_d,
                             void *dxb_d /* optional: bf16 copy of the final dx, row pitch ldb — the dy operand of the next linear backward */,
                             long ldb, void *stream);
size_t lmrl_colsum_ws_bytes(int cols);
int lmrl_colsum(const float *x_d, int rows, int cols, int ld, float *out_d, int accumulate, float *ws_d, void *stream);
/* out[c] (=|+=) sum_r wrow[r * ldw] * x[r][c]: the weight gradient x^T . dy of a Dense layer with ONE output unit (heads/linear_head.py:112-119 as
 * the PPO value head, the V head of heads/mlp_head.py:139-148) — a matrix-vector product; ws_d as for lmrl_colsum. */
int lmrl_colsum_weighted(const float *x_d, int rows, int cols, int ld, const float *wrow_d, int ldw, float *out_d, int accumulate, float *ws_d,
                         void *stream);
/* elementwise ops: in-place calls are supported (y_d == x_d, dx_d == dy_d, out_d == x_d or y_d) */
int lmrl_gelu_fwd(const float *x_d, float *y_d, size_t n, void *stream);
int lmrl_gelu_bwd(const float *dy_d, const float *x_d, float *dx_d, size_t n, void *stream);
/* bf16-matmul mode: dx written only as the bf16 dy operand [rows_dst][ldb] of the next linear backward (padding zero-filled) */
int lmrl_gelu_bwd_bf16(const float *dy_d, const float *x_d, int rows, int cols, void *dst_d, long ldb, int rows_dst, void *stream);
int lmrl_relu_fwd(const float *x_d, float *y_d, size_t n, void *stream);
int lmrl_relu_bwd(const float *dy_d, const float *x_d, float *dx_d, size_t n, void *stream);
/* out = a*x + b*y (y may be NULL).  Polyak: optax.incremental_update(new, old, s) = axpby(s, new, 1-s, old). */
int lmrl_axpby(float a, const float *x_d, float b, const float *y_d, float *out_d, size_t n, void *stream);
/* optax.adamw(b1, b2, eps, weight_decay) with bias correction at `step` (1-based) */
int lmrl_adamw(float *p_d, const float *g_d, float *m_d, float *v_d, size_t n, float lr, float b1, float b2, float eps, float weight_decay,
               int step, void *stream);
/* ---- causal self-attention of the train step without the [B*H][T][T] tensors (csrc/flash_attn_train.hip): online-softmax tile sweeps on the
 * matrix cores, head dim 64.  qkv_d [B*T][3*H*64] fp32 (HF GPT-2 c_attn output: q | k | v), key_mask_d [B][T] uint8 or NULL, att_d / datt_d
 * [B*T][H*64]; lse_d [lmrl_flash_attn_lse_bytes] is written by fwd and read by bwd; ws_d [lmrl_flash_attn_ws_bytes] is scratch (re-staged by
 * each call).  bf16 = 0: exact fp32 operands (v_mfma_f32_16x16x4_f32); 1: bf16 operands, fp32 accumulation / softmax / outputs.
 * Same masking as lmrl_softmax_causal_fwd: keys c <= r with key_mask != 0; a query with no valid key gets a zero output row.
 * Restates the attention of FlaxGPT2 as differentiated by the reference's train steps (ppo/gpt2/interface.py:72-211). */
size_t lmrl_flash_attn_ws_bytes(int batch, int heads, int t, int bf16);
size_t lmrl_flash_attn_lse_bytes(int batch, int heads, int t);
int lmrl_flash_attn_fwd(const float *qkv_d, const uint8_t *key_mask_d, float *att_d, float *lse_d, void *ws_d, int batch, int heads, int t, int bf16,
                        void *stream);
/* forward that also writes the bf16 copy of att (row pitch ldb elements): the operand of the output projection in the bf16-matmul train mode */
int lmrl_flash_attn_fwd_staged(const float *qkv_d, const uint8_t *key_mask_d, float *att_d, float *lse_d, void *ws_d, void *att_bf16_d, long ldb, int batch,
                               int heads, int t, int bf16, void *stream);
/* bf16 workspace: where lmrl_gemm_bf16_qkv_heads writes (q matrix; k and v follow plane_elems apart); lmrl_flash_attn_finish_staging then adds the
 * transposed forms and zeroes the padded token rows, after which lmrl_flash_attn_fwd_staged(qkv_d = NULL, ...) and
 * lmrl_flash_attn_bwd_staged(qkv_d = NULL, ..., qkv_staged = 1) run on ws_d as if they had staged it themselves. */
int lmrl_flash_attn_stage_ptrs(void *ws_d, int batch, int heads, int t, void **q_heads_out, long *plane_elems_out);
int lmrl_flash_attn_finish_staging(void *ws_d, int batch, int heads, int t, void *stream);
int lmrl_flash_attn_bwd(const float *qkv_d, const uint8_t *key_mask_d, const float *att_d, const float *datt_d, const float *lse_d, float *dqkv_d,
                        void *ws_d, int batch, int heads, int t, int bf16,
                        int qkv_staged /* ws_d still holds what lmrl_flash_attn_fwd staged from these qkv: skip the re-staging */, void *stream);
/* bf16 kernels, d(qkv) written only as the bf16 dy operand [batch*t][ldb] of the c_attn backward products (bf16-matmul train mode) */
int lmrl_flash_attn_bwd_staged(const float *qkv_d, const uint8_t *key_mask_d, const float *att_d, const float *datt_d, const float *lse_d,
                               void *dqkv_bf16_d, long ldb, void *ws_d, int batch, int heads, int t, int qkv_staged, void *stream);
/* ... with D = rowsum(dO o O) from the bf16 attention output of lmrl_flash_attn_fwd_staged (att_bf16_d [batch * t][ld_att]); the forward may then be
 * called with att_d = NULL: no fp32 copy of the attention output exists in the bf16-matmul train mode. */
int lmrl_flash_attn_bwd_staged_attb(const float *qkv_d, const uint8_t *key_mask_d, const void *att_bf16_d, long ld_att, const float *datt_d, const float *lse_d,
                                    void *dqkv_bf16_d, long ldb, void *ws_d, int batch, int heads, int t, int qkv_staged, void *stream);
/* ---- dropout of the train step (csrc/dropout.h, dropout.hip; DESIGN.md "Dropout").  Keep masks come from a counter-based stream and are never
 * stored: a forward call has a key (k0, k1); site s (0: embedding output, 1 + 3 l: attention probabilities of block l, 2 + 3 l / 3 + 3 l: output
 * of the attention / MLP c_proj of block l) draws with K_s = threefry2x32(K, (0, s)); element i (row-major in the site's tensor of n < 2^32
 * elements) is kept iff the uniform of word i of jax.random.bits(K_s, (n,)) is < 1 - p, and kept values are multiplied by 1 / (1 - p).
 * lmrl_dropout_host_mask: the keep bytes (1 / 0) of a whole site on the host, for tests without a GPU (p = 0 allowed: all ones). */
int lmrl_dropout_host_mask(uint32_t k0, uint32_t k1, uint32_t site, uint64_t n, float p, uint8_t *out);
/* y = x * mask / (1 - p), 0 < p < 1; y_d may be x_d.  The forward applies it in place; the backward calls it on dy with the same arguments. */
int lmrl_dropout_apply(const float *x_d, float *y_d, uint64_t n, uint32_t k0, uint32_t k1, uint32_t site, float p, void *stream);
/* the same from fp32 x [rows][cols] into the bf16 operand dst [rows_dst][ldb] of a backward product (zero beyond rows / cols), n = rows * cols */
int lmrl_dropout_apply_bf16(const float *x_d, int rows, int cols, void *dst_d, long ldb, int rows_dst, uint32_t k0, uint32_t k1, uint32_t site, float p,
                            void *stream);
/* the flash attention sweeps with dropout on the probabilities (site tensor [batch][heads][t][t]); both arithmetic modes run the generic sweeps.
 * Arguments as lmrl_flash_attn_fwd / _fwd_staged (att_bf16_d NULL: no bf16 copy; att_d NULL in bf16 mode: no fp32 output) and as
 * lmrl_flash_attn_bwd / _bwd_staged / _bwd_staged_attb (exactly one of dqkv_d, dqkv_bf16_d; att_d NULL: D from att_bf16_d).  lse_d is the
 * log-sum-exp of the UNDROPPED scores. */
int lmrl_flash_attn_fwd_dropout(const float *qkv_d, const uint8_t *key_mask_d, float *att_d, float *lse_d, void *ws_d, void *att_bf16_d, long ldb, int batch,
                                int heads, int t, int bf16, uint32_t k0, uint32_t k1, uint32_t site, float p, void *stream);
int lmrl_flash_attn_bwd_dropout(const float *qkv_d, const uint8_t *key_mask_d, const float *att_d, const void *att_bf16_d, long ld_att, const float *datt_d,
                                const float *lse_d, float *dqkv_d, void *dqkv_bf16_d, long ldb, void *ws_d, int batch, int heads, int t, int bf16,
                                int qkv_staged, uint32_t k0, uint32_t k1, uint32_t site, float p, void *stream);
/* ---- bf16-MFMA matmul mode of the train step (csrc/train_bf16.hip): the reference's optional `bf16_activations`
 * (train_ilql_gpt2.py:193; model dtype bf16, fp32 parameters).  Operands are staged as K-major bf16 matrices for lmrl_gemm_bf16.
 * lmrl_cast_bf16: dst [rows_dst][ld_dst] bf16 := round-to-nearest-even of src [rows][cols] fp32 (transpose = 0) or of its transpose
 * (transpose = 1: dst[c][r] = src[r][c]); everything outside the source extent is zero-filled (K padding to multiples of 64). */
int lmrl_cast_bf16(const float *src_d, long ld_src, int rows, int cols, void *dst_d, long ld_dst, int rows_dst, int transpose, void *stream);
/* The bf16 staging of EVERY weight matrix of a parameter arena in one launch (per train step the fp32 masters move: the natural copy [rows][ld_nat]
 * feeds the dX products, the transposed copy [cols][ld_t] the forward products).  Offsets in elements: src_off into src_d (fp32, dense
 * [rows][cols]), nat_off / t_off into dst_d (bf16; < 0: that copy is not wanted); tile0 = number of 64 x 64 tiles of the segments before this one,
 * total_tiles = their sum over all segments.  Only source extents are written — zero-fill dst_d once. */
typedef struct {
    long src_off, nat_off, t_off;
    int rows, cols, ld_nat, ld_t, tile0, pad_;
} lmrl_cast_seg;
int lmrl_cast_bf16_segments(const float *src_d, const lmrl_cast_seg *segs_d, int nseg, int total_tiles, void *dst_d, void *stream);
/* "bf16 x 3" operand of an fp32 matrix: dst [rows][ld_dst >= 3 cols] bf16 := [hi(x) | lo(x) | hi(x)], hi = bf16(x), lo = bf16(x - hi).  Against
 * weight rows [hi(w) | hi(w) | lo(w)], lmrl_gemm_bf16 with K' = 3 cols accumulates hi.hi + lo.hi + hi.lo in fp32: ~16 mantissa bits per product at
 * 3x the bf16 MFMA cost (the f32-input MFMA costs 16x) — the matmul mode "bf16x3" of the fp32 rollout engine (GPT2EngineF32). */
int lmrl_split3_bf16(const float *src_d, long ld_src, int rows, int cols, void *dst_d, long ld_dst, void *stream);
/* transposed cast (as lmrl_cast_bf16 with transpose = 1) that also produces colsum_d[c] (=|+=) sum_r src[r][c] — the bias gradient of a
 * Dense layer falls out of staging dy^T for the dW product instead of a second pass over dy.  ws_d: lmrl_cast_bf16_t_colsum_ws_bytes. */
size_t lmrl_cast_bf16_t_colsum_ws_bytes(int rows, int rows_dst);
int lmrl_cast_bf16_t_colsum(const float *src_d, long ld_src, int rows, int cols, void *dst_d, long ld_dst, int rows_dst, float *colsum_d,
                            int accumulate, float *ws_d, void *stream);
/* bf16-matmul train mode, operands staged by their producer: dlogits of the CE / gather losses (lmrl_ce_bwd's formula) written directly as
 * the bf16 A operand [rows_dst][ld_dst] of the head's backward products (no fp32 dlogits, no cast pass), and the K-major transposed copy
 * (+ optional column sums = the bias gradient, from the bf16 values) made from such a bf16 operand. */
int lmrl_ce_bwd_bf16(const float *logits_d, int ld, int vocab, const float *lse_d, const int32_t *targets_d, const float *coef_ce_d,
                     const float *coef_gather_d, int rows, void *dst_d, long ld_dst, int rows_dst, void *stream);
int lmrl_transpose_bf16_colsum(const void *src_d, long ld_src, int rows, int cols, void *dst_d, long ld_dst, int rows_dst, float *colsum_d,
                               int accumulate, float *ws_d, void *stream);
/* dst[j][i] = beta*dst[j][i] + src[i][j]   (src [n][k] -> dst [k][n]): gradients produced in transposed form */
int lmrl_transpose_add_f32(const float *src_d, long ld_src, float *dst_d, long ld_dst, int n, int k, float beta, void *stream);
/* out[r] = sum_j a[r][j]*w[j][idx[r]] + bias[idx[r]]: the one column of a Dense layer that `take_along_axis(logits, token)` reads —
 * the ILQL target Q heads are only ever evaluated at the taken token (ilql/base_interface.py:57-66), exact fp32 */
int lmrl_gather_dot_f32(const float *a_d, long lda, const float *w_d, long ldw, const float *bias_d, const int32_t *idx_d, float *out_d, int rows,
                        int k, int n, void *stream);
/* lmrl_adamw over a whole parameter arena in one launch: seg_end_d[nseg] (exclusive element ends, ascending, last = n) and seg_wd_d[nseg] give
 * the weight-decay coefficient of each tensor (the optax mask: 0 for biases / LayerNorm).  Element for element the arithmetic of lmrl_adamw. */
int lmrl_adamw_segments(float *p_d, const float *g_d, float *m_d, float *v_d, long n, const long *seg_end_d, const float *seg_wd_d, int nseg, float lr,
                        float b1, float b2, float eps, int step, void *stream);
/* the same update and, in the same sweep, the Polyak target update of the reference's step (optax.incremental_update(new_params, target, alpha) right
 * after apply_gradients, ilql/gpt2/interface.py:327-347): target_d (nullable; same arena layout) = alpha * p_new + one_minus_alpha * target_d.
 * 16-byte accesses; arenas 16-byte aligned. */
int lmrl_adamw_segments_polyak(float *p_d, const float *g_d, float *m_d, float *v_d, long n, const long *seg_end_d, const float *seg_wd_d, int nseg, float lr,
                               float b1, float b2, float eps, int step, float *target_d, float alpha, float one_minus_alpha, void *stream);
/* P = causal (+ key padding mask [batch][t] uint8) softmax of S [batch*heads][t][t]; in place allowed */
int lmrl_softmax_causal_fwd(const float *s_d, const uint8_t *key_mask_d, float *p_d, int batch, int heads, int t, void *stream);
int lmrl_softmax_bwd(const float *p_d, float *dp_d, long rows, int t, void *stream);
/* per row: lse = logsumexp(logits[:vocab]), target logit, logprob = target - lse
 * (= -optax.softmax_cross_entropy_with_integer_labels; PPOInference.token_logprobs_from_logits, ppo/base_interface.py:396-403) */
int lmrl_lse_gather(const float *logits_d, int ld, int vocab, const int32_t *targets_d, float *logprob_d, float *lse_d,
                    float *target_logit_d, int rows, void *stream);
/* logits := coef_ce[r]*(softmax - onehot(t)) + coef_gather[r]*onehot(t)  (CE backward + take_along_axis backward) */
int lmrl_ce_bwd(float *logits_d, int ld, int vocab, const float *lse_d, const int32_t *targets_d, const float *coef_ce_d,
                const float *coef_gather_d, int rows, void *stream);
/* n = sum(should_take_action * attention_mask) as a device double */
int lmrl_mask_sum(const uint8_t *sta_d, const float *attn_d, size_t n, double *out_d, void *stream);
/* ppo_loss_fn forward+backward (ppo/base_interface.py:72-142). partials_d: [lmrl_ppo_loss_blocks(n)][lmrl_ppo_loss_nstats()]
 * doubles (layout in csrc/losses.hip), d_logprobs_d / d_values_d: gradient of the scalar loss. */
int lmrl_ppo_loss_blocks(size_t n);
int lmrl_ppo_loss_nstats(void);
int lmrl_ppo_loss(const float *attn_d, const float *logprobs_d, const float *values_d, const uint8_t *sta_d, const float *old_logprobs_d,
                  const float *old_values_d, const float *old_adv_d, const float *old_ret_d, size_t n, float cliprange_value,
                  float cliprange, float value_loss_coef, const double *n_mask_d, double *partials_d, float *d_logprobs_d,
                  float *d_values_d, void *stream);
/* ilql_loss forward+backward (ilql/base_interface.py:29-119) on gathered q1/q2/v/target-q [b][t1], v_final [b], per-token
 * CQL cross-entropies ce1/ce2 [b][t1]. partials_d: [b][lmrl_ilql_loss_nstats()] doubles. Outputs dq1,dq2,dv,coef_ce [b][t1]. */
int lmrl_ilql_loss_nstats(void);
int lmrl_ilql_loss(const float *q1_d, const float *q2_d, const float *v_d, const float *v_final_d, const float *tq1_d, const float *tq2_d,
                   const float *ce1_d, const float *ce2_d, const float *attn_d, const uint8_t *sta_d, const float *rewards_d, int b, int t1,
                   float gamma, float tau, float cql_weight, const double *n_mask_d, double *partials_d, float *dq1_d, float *dq2_d,
                   float *dv_d, float *coef_ce_d, void *stream);
/* mc_loss forward+backward (mc_returns/base_interface.py:19-60) */
int lmrl_mc_loss_blocks(size_t n);
int lmrl_mc_loss_nstats(void);
int lmrl_mc_loss(const float *q_d, const float *ce_d, const float *attn_d, const uint8_t *sta_d, const float *returns_d, size_t n,
                 float cql_weight, const double *n_mask_d, double *partials_d, float *dq_d, float *coef_ce_d, void *stream);

/* ---- beam search on the device (csrc/beam.hip; the rules of HF-Flax `_beam_search`, transformers 4.26.1, restated in DESIGN.md "Beam search" and
 * unverified against the library).  Per batch item K = num_beams running beams and a pool of K finished hypotheses; rows are item * K + beam.
 * Every buffer is the caller's.  The -1e7 penalties of the rules are carried as flags, never added into a stored value, except in run_score
 * (a beam that was never alive holds -1e7, as the rules initialise it): an UNFLAGGED pool entry stands for fin_score - 1e7.
 * ctl_d: int32 [4][max_new_tokens + 1], zeroed, then ctl[0][0] = 1.  Row 0 is go[t]: position t runs; written for t + 1 by lmrl_beam_select
 * of position t (the loop condition is global over the batch).  Rows 1 - 3 are scratch of lmrl_beam_select.  Every entry below returns at once
 * when its go word is 0, so steps enqueued past the stopping point change nothing. */
typedef struct {
    float *run_score;     /* [b K]      sum of log-probabilities of the running beams, descending per item; initially {0, -1e7, ...} */
    int32_t *run_hist;    /* [b K][cap] their generated tokens */
    float *fin_score;     /* [b K]      finished pool: score / length ** length_penalty (unpenalised); initially 0 */
    uint8_t *fin_flag;    /* [b K]      1: a hypothesis that ended in eos; initially 0 */
    int32_t *fin_hist;    /* [b K][cap] tokens of the pool entries, pad_token behind the last */
} lmrl_beam_state;
/* One workgroup per row, one pass over logits_d [rows][ld] (ld % 4 == 0, 16-byte aligned) with 16-byte loads: log-sum-exp over columns [0, vocab)
 * and the row's n_cand (<= min(32, vocab)) largest logits there, ties to the lower column -> cand_score_d [rows][n_cand] = logit - lse +
 * running_score_d[row] in descending order, cand_tok_d [rows][n_cand] their columns.  Columns >= vocab are never looked at.  active_d (NULL: all):
 * rows with 0 are skipped; go_d (NULL: run): one word. */
int lmrl_beam_row_topk(const float *logits_d, int ld, int rows, int vocab, int n_cand, const float *running_score_d, const uint8_t *active_d,
                       const int32_t *go_d, float *cand_score_d, int32_t *cand_tok_d, void *stream);
/* One wave per item, position t (0-based) of the generation: with the candidates of lmrl_beam_row_topk at n_cand = 2 num_beams (num_beams <= 16,
 * vocab >= 2 num_beams) — the item's top 2K by score (ties: lower beam * vocab + token); the next running beams = those candidates in rank order,
 * eos candidates behind all others; the finished pool = top K of [pool | candidates] by (unpenalised first, score / norm_div, lower merged
 * index), candidates penalised unless they end in eos_token (< 0: none), all of them when the pool was full and early_stopping is set.  `in` is
 * read, `out` written (two states, no shared buffer).  parent_d [b K]: absolute row whose cache each new running beam continues; next_tok_d /
 * next_cnt_d [b K]: the inputs of the next single-token forward (next_cnt_d = 1; all 0 once go[t + 1] is 0).  norm_div = (prompt width + t) **
 * length_penalty, best_div = (prompt width + max_new_tokens) ** length_penalty: go[t + 1] = t + 1 < max_new_tokens, and not (every pool of the
 * batch full and early_stopping), and some item has a beam whose worst_finished (the pool's minimum where the beam's entry is flagged, -1e7
 * elsewhere) lies below run_score[best_running_beam] / best_div. */
int lmrl_beam_select(const lmrl_beam_state *in, const lmrl_beam_state *out, const float *cand_score_d, const int32_t *cand_tok_d, int32_t *parent_d,
                     int32_t *next_tok_d, int32_t *next_cnt_d, int32_t *ctl_d, int b, int num_beams, int vocab, int cap, int t, int max_new_tokens,
                     int eos_token, int pad_token, int early_stopping, int best_running_beam, float norm_div, float best_div, void *stream);
/* The caches follow the beams: for every layer, K and V of positions [from_d[i] (NULL: 0), src_len_d[parent_d[i]]) of source row parent_d[i] go to
 * row i of a SECOND cache of the same shape (b rows of tmax positions), dst_len_d[i] = src_len_d[parent_d[i]], and the last hidden state (the fp32
 * form: and the last residual) is copied.  from_d = pfx_n_d of the attach call: the prompt's rows stay where they are.  One launch for all layers. */
int lmrl_gpt2_kv_reorder(const lmrl_gpt2 *m, const void *src_kv_d, const int32_t *src_len_d, const void *src_hidden_d, const int32_t *parent_d,
                         const int32_t *from_d, void *dst_kv_d, int32_t *dst_len_d, void *dst_hidden_d, int b, int tmax, const int32_t *go_d,
                         void *stream);
int lmrl_kv_reorder_f32(const float *src_kv_d, const int32_t *src_len_d, const float *src_hidden_d, const float *src_last_x_d, const int32_t *parent_d,
                        const int32_t *from_d, float *dst_kv_d, int32_t *dst_len_d, float *dst_hidden_d, float *dst_last_x_d, int b, int tmax, int n_layer,
                        int d, const int32_t *go_d, void *stream);

/* ------------------------------------------------------------------------------------------
 * GPT-J on the fp32 rollout mode (csrc/attn_rope_f32.hip; `lmrl_gym_amd.gptj_f32_engine.GPTJEngineF32` sequences these with lmrl_sgemm,
 * lmrl_layernorm_*, lmrl_gelu_fwd and the lmrl_chunk_*_f32 calls above).
 *   lmrl_rope_gptj_f32   GPT-J's rotary embedding ("rotate every two"), in place on q and k of qkv_d fp32 [rows][3 * n_head * head_dim]: for pair
 *                        i < rotary_dim / 2 of every head,  y[2i] = x[2i] cos - x[2i+1] sin,  y[2i+1] = x[2i+1] cos + x[2i] sin  with
 *                        sin = sincos_d[pos][i], cos = sincos_d[pos][rotary_dim / 2 + i]; sincos_d fp32 [n_pos][rotary_dim] = [sin | cos] is built by
 *                        the host (HF `create_sinusoidal_positions`).  v, dims >= rotary_dim and rows with pos_d[row] < 0 are not touched.
 *                        rotary_dim even, <= head_dim.  The positions are read back and checked first (one stream synchronisation): a row with
 *                        pos >= n_pos is LMRL_ERR_ARG and nothing is launched.  Not usable inside a stream capture (LMRL_ERR_ARG).
 *   lmrl_rope_gptj_f32_async  the same launch without the read-back (no synchronisation: capturable).  The kernel itself never reads the table
 *                        for a row with pos >= n_pos — such a row passes through unrotated — so the caller has to bound the positions
 *                        (GPTJEngineF32 does, on the host, from its cache-length bound).
 *   lmrl_attn_cached_hd_f32  lmrl_attn_cached_f32 with the head dim passed in, head_dim in {64, 128, 256} (else LMRL_ERR_ARG): same cache layout
 *                        ([b][tmax][n_head * head_dim]) and arguments, scores scaled by 1 / sqrt(head_dim), one launch for any c (chunk and
 *                        decode).  One wave per (env, head, query); keys walked in tiles of lmrl_attn_hd_key_tile() positions; online softmax and
 *                        accumulation in fp32.  An env whose new rows do not fit (len + j >= tmax) is skipped.
 * ------------------------------------------------------------------------------------------ */
int lmrl_rope_gptj_f32(float *qkv_d, const int32_t *pos_d, const float *sincos_d, int rows, int n_head, int head_dim, int rotary_dim, int n_pos,
                       void *stream);
int lmrl_rope_gptj_f32_async(float *qkv_d, const int32_t *pos_d, const float *sincos_d, int rows, int n_head, int head_dim, int rotary_dim, int n_pos,
                             void *stream);
int lmrl_attn_cached_hd_f32(const float *qkv_d, float *kcache_d, float *vcache_d, const int32_t *len_d, const int32_t *cnt_d, float *out_d, int b, int c,
                            int n_head, int head_dim, int tmax, void *stream);
int lmrl_attn_hd_key_tile(void);

#ifdef __cplusplus
}
#endif
#endif /* LMRL_AMD_H */
