// wordle_policy_core.h — scalar logic of the scripted Wordle policies (host + device).
//
// Reference: llm_rl_scripts/wordle/env/scripted_policies.py (RandomMixturePolicy :114-126, OptimalPolicy :66-96,
// StartWordPolicy :42-64, MixturePolicy :143-153) on the knowledge state of wordle_core.h.
//
// OptimalPolicy scores every word g of the filtered list (file order) by
//     info_gain(g) = log(F) - (sum over groups of log(size(next_state)) * count) / F
// where the filtered targets are grouped by the knowledge state that guessing g would produce, the groups are visited in
// order of first occurrence, and everything is float64 in exactly that operation order (ties between words are the common
// case, so the sum has to come out to the last bit).  Two facts about a state S that some vocabulary word satisfies, and a
// target t that satisfies S, carry the implementation (proof sketch; tests/test_wordle_policies.py checks both against the
// literal definition on every fixture state and on >= 10 000 further reachable states):
//
//  (1) T(S, g, t) is determined by S, g and the 3^5 feedback pattern of g against t, and two targets with different patterns
//      give different states.  Every per-letter operation of the transition only adds knowledge that t satisfies (a HERE is
//      never put on a NOT_HERE that t contradicts, a letter S requires never becomes all-NOT_HERE), so any word w that
//      satisfies N = T(S, g, t) also satisfies S, and at each position of g the knowledge N holds about that letter forces
//      w's own feedback symbol: w has the same pattern as t.  Hence <= 243 groups, keyed by pattern.
//  (2) For the same reason {w in V : w satisfies N} = {w in filtered(S) : pattern(g, w) = pattern(g, t)}: the reference's
//      `next_state.vocab.filtered_vocab_size()` equals the group's own count, so no second pass over the vocabulary is needed.
#pragma once
#include "mt19937.h"
#include "wordle_core.h"

namespace lmrl {

constexpr int kWordlePatterns = 243;      // 3^5
constexpr int kWordleMaxStartWords = 64;

enum { kWordlePolMixture = 0, kWordlePolOptimal = 1 };

// Feedback symbol of guess letter i against a target: 0 correct_pos, 1 wrong_pos, 2 not_used (game.py:85-91).
LMRL_HD uint32_t wordle_pattern(uint32_t guess, uint32_t target, uint32_t tmask) {
    uint32_t p = 0, pw = 1;
    for (int i = 0; i < 5; i++) {
        const uint32_t c = letter_at(guess, i);
        const uint32_t sym = (c == letter_at(target, i)) ? 0u : (((tmask >> c) & 1u) ? 1u : 2u);
        p += sym * pw;
        pw *= 3u;
    }
    return p;
}

// WordleState.transition_from_str (game.py:94-107) for one action: `code` in the encoding of wordle_obs
// (bits [3k,3k+3) = k-th symbol 1 g / 2 y / 3 b, bits [16,19) = number of symbols).  Returns false when the code does not carry
// five symbols (the reference raises there).
LMRL_HD bool wordle_apply_feedback(WordleMasks &s, uint32_t guess, uint32_t code) {
    if (((code >> 16) & 7u) != 5u) return false;
    for (int i = 0; i < 5; i++) {
        const uint32_t bit = 1u << letter_at(guess, i);
        const uint32_t sym = (code >> (3 * i)) & 7u;
        if (sym == 1u) {
            s.must[i] |= bit;
            s.forb[i] &= ~bit;
        } else if (sym == 2u) {
            s.forb[i] |= bit;
            s.must[i] &= ~bit;
        } else if (sym == 3u) {
            for (int k = 0; k < 5; k++) {
                s.forb[k] |= bit;
                s.must[k] &= ~bit;
            }
        } else {
            return false;
        }
    }
    wordle_derive(s);
    return true;
}

// One term of `total_entropy += math.log(size) * state_count` and the closing `math.log(F) - total_entropy / total`
// (scripted_policies.py:88-90).  logtab[k] = math.log(k) as CPython computes it, filled by the host.  Separate multiply, add and
// divide: the build passes -ffp-contract=off.
LMRL_HD double wordle_gain_add(double acc, uint32_t size, uint32_t count, const double *logtab) {
    const double term = logtab[size] * (double)count;
    return acc + term;
}
LMRL_HD double wordle_gain_finish(double acc, uint32_t total, const double *logtab) {
    const double mean = acc / (double)total;
    return logtab[total] - mean;
}

LMRL_HD bool wordle_is_initial(const WordleMasks &s) {
    uint32_t any = 0;
    for (int i = 0; i < 5; i++) any |= s.forb[i] | s.must[i];
    return any == 0;
}

// ---- serial forms (host faces, and the device's one-lane corner cases)

// Vocabulary filter in file order (game.py:154); returns F.
inline int wordle_filtered_list(const WordleMasks &s, const uint32_t *words, int V, int32_t *idx) {
    int f = 0;
    for (int i = 0; i < V; i++)
        if (wordle_consistent(s, words[i], letters_mask(words[i]))) idx[f++] = i;
    return f;
}

// info gain of guess `g` over the filtered list, pattern buckets + count-as-size (facts 1 and 2 above)
inline double wordle_gain_buckets(uint32_t g, const uint32_t *words, const int32_t *idx, int F, const double *logtab) {
    uint32_t cnt[kWordlePatterns];
    int order[kWordlePatterns];
    int n_groups = 0;
    for (int p = 0; p < kWordlePatterns; p++) cnt[p] = 0;
    for (int j = 0; j < F; j++) {
        const uint32_t t = words[idx[j]];
        const uint32_t p = wordle_pattern(g, t, letters_mask(t));
        if (cnt[p]++ == 0) order[n_groups++] = (int)p;
    }
    double acc = 0.0;
    for (int k = 0; k < n_groups; k++) acc = wordle_gain_add(acc, cnt[order[k]], cnt[order[k]], logtab);
    return wordle_gain_finish(acc, (uint32_t)F, logtab);
}

// the literal definition: group by the next knowledge state itself (first occurrence order), size = filter of that state over the
// WHOLE vocabulary (game.py:224-232, scripted_policies.py:87-90).  `groups` is caller scratch of F entries.
struct WordleGroup {
    WordleMasks s;
    uint32_t count;
};
inline double wordle_gain_literal(const WordleMasks &s, uint32_t g, const uint32_t *words, int V, const int32_t *idx, int F,
                                  const double *logtab, WordleGroup *groups) {
    int n_groups = 0;
    for (int j = 0; j < F; j++) {
        WordleMasks nx = s;
        wordle_transition(nx, g, words[idx[j]]);
        int k = 0;
        for (; k < n_groups; k++) {
            bool same = true;
            for (int i = 0; i < 5; i++) same = same && groups[k].s.forb[i] == nx.forb[i] && groups[k].s.must[i] == nx.must[i];
            if (same) break;
        }
        if (k == n_groups) {
            groups[n_groups].s = nx;
            groups[n_groups].count = 0;
            n_groups++;
        }
        groups[k].count++;
    }
    double acc = 0.0;
    uint32_t total = 0;
    for (int k = 0; k < n_groups; k++) {
        uint32_t size = 0;
        for (int i = 0; i < V; i++) size += wordle_consistent(groups[k].s, words[i], letters_mask(words[i])) ? 1u : 0u;
        acc = wordle_gain_add(acc, size, groups[k].count, logtab);
        total += groups[k].count;
    }
    return wordle_gain_finish(acc, total, logtab);
}

}  // namespace lmrl
