// tq_core.h — the per-env text rules of Twenty Questions as plain functions over byte buffers (host + device).
//
// What `BatchedTwentyQuestionsPolicyEnvironment.step` does to one slot's strings per turn (lmrl-gym_amd/envs/twenty_questions.py; the reference:
// llm_rl_scripts/twenty_questions/env/{env,data,oracle}.py), for tokenizers whose ids ARE the text's UTF-8 bytes:
//   generated ids -> text (`decode(ids, skip_special_tokens=True)`: UTF-8 with errors="ignore") -> the PPO script's `out_str_process`
//     (`removesuffix('\n') + '\n'`) -> the question as the history holds it -> Python `str.strip()` of it -> the text the oracle is asked;
//   the oracle's generated ids -> text -> `strip().lower()` -> `re.match("(yes|no)")` -> "Yes." / "No." (`answers_from_outputs`);
//   `is_done(word, question)` with the stand-in tagger `rule_pos_tag`, for questions made of code points < 0x80.
// The closed word lists of the tagger (determiners, function words, generic nouns) and every spelling's token list come from Python in one
// string table (`TqTables`); nothing of them is restated here.
#pragma once
#include <stdint.h>

#ifdef LMRL_HOST_ONLY
#define LMRL_HD inline
#else
#include <hip/hip_runtime.h>
#define LMRL_HD __host__ __device__ __forceinline__
#endif

namespace lmrl_tq {

// One string table: string s = bytes [str_off[s], str_off[s + 1]).  Strings [0, n_det) are the determiners, [n_det, n_det + n_func) the function
// words, the next n_generic the generic nouns; behind them the lower-cased tokens of every spelling of every word, spelling by spelling:
// spelling p = strings [spell_off[p], spell_off[p + 1]), word w = spellings [word_off[w], word_off[w + 1]).
struct TqTables {
    const uint8_t *bytes;
    const int32_t *str_off, *spell_off, *word_off;
    int n_det, n_func, n_generic, n_words;
    const uint8_t *tok_blen;          // [vocab] 0: the id adds nothing to the text (special ids)
    int vocab, eos;                   // eos < 0: none
    const uint8_t *invalid_q;         // INVALID_QUESTION as bytes
    int invalid_q_len;
};

// Python's str.isspace() per code point (what str.strip() removes; for < 0x80 also what `\s` matches in a str pattern)
LMRL_HD bool py_space(int cp) {
    return (cp >= 9 && cp <= 13) || (cp >= 28 && cp <= 32) || cp == 0x85 || cp == 0xA0 || cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) || cp == 0x2028 ||
           cp == 0x2029 || cp == 0x202F || cp == 0x205F || cp == 0x3000;
}
LMRL_HD bool is_alpha(int c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
LMRL_HD bool is_digit(int c) { return c >= '0' && c <= '9'; }
LMRL_HD int lower(int c) { return (c >= 'A' && c <= 'Z') ? c + 32 : c; }

// ids up to and including the first eos -> the bytes of `decode(ids, skip_special_tokens=True)`: ids outside 0..255 and special ids add nothing,
// the byte stream is decoded as UTF-8 with errors="ignore" (an invalid start byte is dropped alone; a sequence broken at byte k drops the bytes
// read so far and decoding resumes AT the offending byte; a sequence cut by the end of the data is dropped).  out: cap bytes.  -> length
LMRL_HD int text_from_ids(const TqTables &T, const int32_t *ids, int n, uint8_t *out, int cap) {
    if (T.eos >= 0)
        for (int i = 0; i < n; i++)
            if (ids[i] == T.eos) { n = i + 1; break; }
    int raw = 0;                                              // pass 1: the byte stream, in place in `out`
    for (int i = 0; i < n && raw < cap; i++) {
        const int t = ids[i];
        if (t < 0 || t >= 256) continue;
        if (t < 128 && t < T.vocab && T.tok_blen[t] == 0) continue;      // an ASCII byte the tokenizer declares special
        out[raw++] = (uint8_t)t;
    }
    int len = 0, i = 0;                                       // pass 2: keep the valid sequences (len <= i always)
    while (i < raw) {
        const int b0 = out[i];
        if (b0 < 0x80) { out[len++] = (uint8_t)b0; i++; continue; }
        if (b0 < 0xC2 || b0 > 0xF4) { i++; continue; }
        const int need = b0 < 0xE0 ? 1 : (b0 < 0xF0 ? 2 : 3);
        int lo = 0x80, hi = 0xBF;                             // range of the second byte (no overlongs, no surrogates, <= U+10FFFF)
        if (b0 == 0xE0) lo = 0xA0; else if (b0 == 0xED) hi = 0x9F; else if (b0 == 0xF0) lo = 0x90; else if (b0 == 0xF4) hi = 0x8F;
        int got = 0;
        for (; got < need; got++) {
            if (i + 1 + got >= raw) break;
            const int b = out[i + 1 + got];
            if (got == 0 ? (b < lo || b > hi) : (b < 0x80 || b > 0xBF)) break;
        }
        if (got < need) { i += 1 + got; continue; }
        for (int k = 0; k <= need; k++) out[len++] = out[i + k];
        i += need + 1;
    }
    return len;
}

// the code point that starts at s[i] of VALID UTF-8 (-> its byte count in *nb)
LMRL_HD int cp_at(const uint8_t *s, int i, int *nb) {
    const int b0 = s[i];
    if (b0 < 0x80) { *nb = 1; return b0; }
    if (b0 < 0xE0) { *nb = 2; return ((b0 & 0x1F) << 6) | (s[i + 1] & 0x3F); }
    if (b0 < 0xF0) { *nb = 3; return ((b0 & 0x0F) << 12) | ((s[i + 1] & 0x3F) << 6) | (s[i + 2] & 0x3F); }
    *nb = 4;
    return ((b0 & 0x07) << 18) | ((s[i + 1] & 0x3F) << 12) | ((s[i + 2] & 0x3F) << 6) | (s[i + 3] & 0x3F);
}

// Python str.strip() of valid UTF-8: the kept byte range [*begin, *end)
LMRL_HD void py_strip(const uint8_t *s, int n, int *begin, int *end) {
    int b = 0, e = n, nb;
    while (b < e && py_space(cp_at(s, b, &nb))) b += nb;
    while (e > b) {
        int k = e - 1;
        while (k > b && (s[k] & 0xC0) == 0x80) k--;          // back to the lead byte
        if (!py_space(cp_at(s, k, &nb))) break;
        e = k;
    }
    *begin = b; *end = e;
}

// generated ids -> the question as the history holds it (`out_str_process`: exactly one trailing newline ensured) and the range of its strip().
// q: cap bytes, cap >= n + 1.  -> length of the question
LMRL_HD int question_from_ids(const TqTables &T, const int32_t *ids, int n, uint8_t *q, int cap, int *begin, int *end) {
    int len = text_from_ids(T, ids, n, q, cap - 1);
    if (len > 0 && q[len - 1] == '\n') len--;
    q[len++] = '\n';
    py_strip(q, len, begin, end);
    return len;
}

// `answers_from_outputs` for one row -> 1 "Yes." / 0 "No.": INVALID_QUESTION is answered "No." unread; else strip().lower() must start with yes / no
// (only ASCII letters lower-case to y, e, s, n, o).  `scratch`: cap bytes for the decoded text.
LMRL_HD int answer_from_ids(const TqTables &T, const uint8_t *question, int qn, const int32_t *ids, int n, uint8_t *scratch, int cap) {
    if (qn == T.invalid_q_len) {
        bool same = true;
        for (int i = 0; i < qn && same; i++) same = question[i] == T.invalid_q[i];
        if (same) return 0;
    }
    const int len = text_from_ids(T, ids, n, scratch, cap);
    int b, e;
    py_strip(scratch, len, &b, &e);
    return e - b >= 3 && lower(scratch[b]) == 'y' && lower(scratch[b + 1]) == 'e' && lower(scratch[b + 2]) == 's';
}

// ---- rule_pos_tag on ASCII text.  Tokens: runs of [A-Za-z0-9'] or single characters that are neither blank nor in that class.
LMRL_HD bool word_char(int c) { return is_alpha(c) || is_digit(c) || c == '\''; }
LMRL_HD bool next_token(const uint8_t *s, int n, int *pos, int *ts, int *tl) {
    int i = *pos;
    while (i < n && py_space(s[i])) i++;
    if (i >= n) { *pos = i; return false; }
    *ts = i;
    if (word_char(s[i])) { while (i < n && word_char(s[i])) i++; } else i++;
    *tl = i - *ts;
    *pos = i;
    return true;
}
// token (lower-cased on the fly) == table string k
LMRL_HD bool tok_is(const TqTables &T, const uint8_t *s, int ts, int tl, int k) {
    const int a = T.str_off[k];
    if (T.str_off[k + 1] - a != tl) return false;
    for (int i = 0; i < tl; i++)
        if (lower(s[ts + i]) != T.bytes[a + i]) return false;
    return true;
}
LMRL_HD bool tok_in(const TqTables &T, const uint8_t *s, int ts, int tl, int k0, int k1) {
    for (int k = k0; k < k1; k++)
        if (tok_is(T, s, ts, tl, k)) return true;
    return false;
}
// tagged NN / NNS: starts with a letter or digit, is not a number, not a determiner, not a function word
LMRL_HD bool is_noun(const TqTables &T, const uint8_t *s, int ts, int tl) {
    if (s[ts] == '\'') return false;
    if (!word_char(s[ts])) return false;
    bool digits = true;
    for (int i = 0; i < tl && digits; i++) digits = is_digit(s[ts + i]);
    if (digits) return false;
    return !tok_in(T, s, ts, tl, 0, T.n_det + T.n_func);
}

// `is_done(word_list[word], question)` under rule_pos_tag.  *judgeable = 0 (and false) for a question with a byte >= 0x80: not decided here.
LMRL_HD bool is_done(const TqTables &T, int word, const uint8_t *q, int n, int *judgeable) {
    *judgeable = 1;
    for (int i = 0; i < n; i++)
        if (q[i] >= 0x80) { *judgeable = 0; return false; }
    int end = n;
    while (end > 0 && !is_alpha(q[end - 1])) end--;          // the trailing punctuation / blanks / digits are dropped
    if (end == 0) return false;
    const int generic0 = T.n_det + T.n_func, generic1 = generic0 + T.n_generic;
    const int sp0 = T.word_off[word], sp1 = T.word_off[word + 1];
    const int w0 = T.spell_off[sp0], w1 = T.spell_off[sp1];  // every token of every spelling of the word
    int n_tok = 0, pos = 0, ts, tl;
    while (next_token(q, end, &pos, &ts, &tl)) {
        n_tok++;
        if (!is_noun(T, q, ts, tl) || tok_in(T, q, ts, tl, generic0, generic1) || tok_in(T, q, ts, tl, w0, w1)) continue;
        int p2 = pos, ts2, tl2;                               // a counter noun directly followed by "of" is no stray noun
        if (next_token(q, end, &p2, &ts2, &tl2) && tl2 == 2 && lower(q[ts2]) == 'o' && lower(q[ts2 + 1]) == 'f') continue;
        return false;
    }
    for (int sp = sp0; sp < sp1; sp++) {                      // the question must END with the token sequence of one spelling
        const int k0 = T.spell_off[sp], len = T.spell_off[sp + 1] - k0;
        if (len > n_tok) continue;
        pos = 0;
        for (int i = 0; i < n_tok - len; i++) next_token(q, end, &pos, &ts, &tl);
        bool same = true;
        for (int i = 0; i < len && same; i++) {
            next_token(q, end, &pos, &ts, &tl);
            same = tok_is(T, q, ts, tl, k0 + i);
        }
        if (same) return true;
    }
    return false;
}

}  // namespace lmrl_tq
