// wordle_ctx.h — the Wordle context object and the game-state buffer layout, shared by wordle.hip (env) and
// wordle_policy.hip (scripted policies, episode loop).
#pragma once
#include <stdint.h>

namespace lmrl {

struct WordleCtx {
    uint32_t *words_d = nullptr;   // [V] packed 5x5-bit letters, file order
    uint32_t *wmask_d = nullptr;   // [V] 26-bit letter-presence masks
    int V = 0;
    int require = 1;
    float bad_reward = -1.f;
    int step_variant = 0;          // 0: by batch size, 1: one wave per env, 2: one lane per env (lmrl_wordle_set_variant)
};

// rows of the SoA game-state buffer
enum { ROW_FORB = 0, ROW_MUST = 5, ROW_NFILT = 10, ROW_NACT = 11, ROW_HIST = 12 };

}  // namespace lmrl

struct lmrl_wordle_ctx : public lmrl::WordleCtx {};
