// wordle_accept_core.h — per-env bookkeeping of one sampled action token (the body of tok_accept_kernel, csrc/wordle_tokens.hip), shared with
// the fused reduce + accept + embed launch of the Wordle rollout (csrc/gpt2.hip), and the token context both read.
#pragma once
#include "../../include/lmrl_amd.h"
#include <stdint.h>

namespace lmrl {

struct WordleTokCtx {
    lmrl_wordle_tokens t;
    uint32_t *cls_d = nullptr;   // [vocab] token classes
    int vocab = 0, max_new = 0, cap = 0;
};

// k-th sampled token `tok` of env e's current action: record it; eos / max_new_tokens end the action.  One thread per env.
// Returns the env's count for the next single-token forward (1: `tok` goes on through the model, 0: nothing).
__device__ __forceinline__ int wordle_accept_env(const lmrl_wordle_traj &tr, int e, int tok, int k, int max_new, int newline,
                                                 int32_t *__restrict__ next_tok, int32_t *__restrict__ next_cnt, uint8_t *__restrict__ active_out) {
    int cnt = 0;
    if (tr.gen_active[e]) {
        tr.gen[(size_t)e * max_new + k] = tok;
        tr.gen_len[e] = k + 1;
        if (tok == newline || k + 1 >= max_new) tr.gen_active[e] = 0;   // eos reached or max_new_tokens
        else { cnt = 1; next_tok[e] = tok; }
    }
    next_cnt[e] = cnt;
    if (active_out) active_out[e] = (uint8_t)cnt;
    return cnt;
}

}  // namespace lmrl

struct lmrl_wordle_tok_ctx : public lmrl::WordleTokCtx {};
