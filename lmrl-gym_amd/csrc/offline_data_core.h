// offline_data_core.h — one scripted Wordle episode -> its token trajectory, slot by slot (host + device).
//
// Reference: the jsonl items of llm_rl_scripts/wordle/misc/data_gen.py:53-62 (the REFORMATTED history of env.py:7-17: header 'Wordle:\n',
// actions 'a b c d e\n', observations 'g y b b y\n' or '\n') tokenised by TokenTrajectory.from_text_trajectory (LLM_RL/environment.py:349-380):
// every text's tokens carry the text's is_action flag, a text's reward sits on its LAST token, 0 elsewhere.  The rewards of an item are
// [0 (header)] + [r, 0] per turn (train_ilql_gpt2.py:123-134), so r lands on the '\n' that closes the action.
//
// An episode is (guess, obs, reward)[6] + n_turns as lmrl_wordle_policy_episodes records it.  Token slot s of the row is a pure function of
// the episode, which is what lets a wave spread one episode over its lanes: the header takes n_header slots, turn k takes 6 action slots and
// (symbols + 1) observation slots.
#pragma once
#include "../../include/lmrl_amd.h"
#include "wordle_core.h"

namespace lmrl {

struct WordleEpisode {
    uint32_t guess[kWordleTries], obs[kWordleTries];
    float reward[kWordleTries];
    int n_turns;
};

LMRL_HD int wordle_obs_symbols(uint32_t code) {
    const int ns = (int)((code >> 16) & 7u);
    return ns > 5 ? 5 : ns;
}

// tokens of the whole episode
LMRL_HD int wordle_episode_ntok(const lmrl_wordle_tokens &t, const WordleEpisode &e) {
    int n = t.n_header;
    for (int k = 0; k < e.n_turns; k++) n += 6 + wordle_obs_symbols(e.obs[k]) + 1;
    return n;
}

// token / is_action / reward of slot `s`; false past the episode's last token (nothing written)
LMRL_HD bool wordle_episode_slot(const lmrl_wordle_tokens &t, const WordleEpisode &e, int s, int32_t &tok, uint8_t &ia, float &rw) {
    if (s < 0) return false;
    if (s < t.n_header) {
        tok = t.header[s]; ia = 0; rw = 0.f;
        return true;
    }
    int off = t.n_header;
    for (int k = 0; k < e.n_turns; k++) {
        const int ns = wordle_obs_symbols(e.obs[k]);
        const int j = s - off;
        if (j < 6) {                              // 'a b c d e\n': the turn's reward on the closing newline
            if (j < 5) {
                const uint32_t c = letter_at(e.guess[k], j) % 26u;
                tok = j == 0 ? t.letter_first[c] : t.letter_sp[c];
            } else {
                tok = t.newline;
            }
            ia = 1; rw = j == 5 ? e.reward[k] : 0.f;
            return true;
        }
        if (j < 6 + ns + 1) {                     // 'g y b b y\n', or '\n' alone when the env returned no symbols
            const int i = j - 6;
            if (i < ns) {
                int sym = (int)((e.obs[k] >> (3 * i)) & 7u) - 1;      // 0 g, 1 y, 2 b
                sym = sym < 0 ? 0 : (sym > 2 ? 2 : sym);
                tok = i == 0 ? t.sym_first[sym] : t.sym_sp[sym];
            } else {
                tok = t.newline;
            }
            ia = 0; rw = 0.f;
            return true;
        }
        off += 6 + ns + 1;
    }
    return false;
}

}  // namespace lmrl
