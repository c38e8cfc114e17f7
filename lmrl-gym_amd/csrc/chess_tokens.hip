// chess_tokens.hip — on-device token <-> game bookkeeping for lock-step chess rollouts (configs[3]: chess/ppo/train_ppo_gpt2_online.py:201-340).
//
// The reference's act()/step() cycle for the chess env (LLM_RL/environment.py:180-206, ppo/gpt2/interface.py:519-546, chess/env/env.py:91-238)
// renders `' '.join(board.fen())`, tokenises it, generates, decodes the ids, applies `out_str_process` and `postprocess_move`, pushes the SAN
// string, asks the opponent for a reply and renders the next FEN.  The rules already run on the device (chess_rules.h, one game per lane); this
// file adds the text <-> token layer around them so that a turn is
//   kept prompt prefix | FEN bytes -> prompt ids (16-token chunks) | generate | ids -> SAN bytes -> agent half-step | opponent pick + half-step | record
// with no host round trip (device opponent), or with one [B][8] hand-off of UCI moves each way (host engine pool).
// Integer / byte work, one game per lane like chess.hip; a game's Pos and move list live in private memory; nothing here needs LDS.
#include "../../include/lmrl_amd.h"
#include "common.h"
#include "chess_rules.h"
#include <string.h>

using namespace lmrl_chess;

struct lmrl_chess_tok_ctx {
    int32_t *byte_id_d = nullptr;          // [256] id of every single byte (-1: the tokenizer has none)
    uint8_t *tok_bytes_d = nullptr, *tok_blen_d = nullptr;
    int32_t byte_id_h[256];
    uint8_t *tok_bytes_h = nullptr, *tok_blen_h = nullptr;
    int vocab = 0, byte_ids = 0, eos = -1, max_new = 0, max_turns = 0;
};

namespace lmrl {

constexpr int kCFen = LMRL_CHESS_FEN_BYTES, kCAct = LMRL_CHESS_ACTION_BYTES;
constexpr int kCTokBytes = 16;         // byte-table pitch (token_byte_table of maze_rollout.py)

// ---- Philox4x32-7: the function of csrc/sampler.hip (same multipliers, key schedule and round count), restated for the reply stream
LMRL_HD inline uint32_t chess_philox_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 7; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

struct TokTables {
    const int32_t *byte_id;
    const uint8_t *tok_bytes, *tok_blen;
    int vocab, byte_ids, eos;
};

// ---- the decoded text of a generation, character by character: `tokenizer.decode(ids, skip_special_tokens=True)`.
// Two tokenizer kinds.  byte_ids (ids 0..255 ARE the text's UTF-8 bytes; other ids decode to nothing): the byte stream goes through a UTF-8
// decoder with Python's errors="ignore" rule (an invalid start byte is dropped alone; a sequence broken at byte k drops its first k bytes and
// decoding resumes AT the offending byte; a sequence cut by the end of the data is dropped).  Otherwise: the per-token byte table — length 0 =
// skipped (special ids), 255 = a token that is not ASCII text: one character that is neither blank nor ASCII.
struct Ch {
    int cp;                 // code point; -1 = end of text; 0x110000 = "some non-ASCII, non-blank character" (table mode)
    uint8_t b[4];           // its UTF-8 bytes
    int nb;
};

struct CharIter {
    const TokTables &T;
    const int32_t *ids;
    int n, k = 0, q = 0;
    LMRL_HD CharIter(const TokTables &t, const int32_t *i, int len) : T(t), ids(i), n(len) {}
    // byte mode: the byte at or after token kk (skipping ids that decode to nothing); -1 at the end.  kk is left ON that token.
    LMRL_HD int peek(int &kk) const {
        for (; kk < n; kk++) {
            const int t = ids[kk];
            if (t < 0 || t >= 256) continue;
            if (t < 128 && t < T.vocab && T.tok_blen[t] == 0) continue;      // an ASCII byte the tokenizer declares special
            return t;
        }
        return -1;
    }
    LMRL_HD static bool cont(int b) { return b >= 0x80 && b <= 0xBF; }
    LMRL_HD Ch next() {
        Ch c; c.cp = -1; c.nb = 0;
        if (!T.byte_ids) {
            while (k < n) {
                const int t = ids[k];
                const int bl = (t >= 0 && t < T.vocab) ? T.tok_blen[t] : 255;
                if (bl == 0) { k++; q = 0; continue; }
                if (bl == 255) { k++; q = 0; c.cp = 0x110000; return c; }
                c.cp = T.tok_bytes[(size_t)t * kCTokBytes + q]; c.b[0] = (uint8_t)c.cp; c.nb = 1;
                if (++q >= bl) { k++; q = 0; }
                return c;
            }
            return c;
        }
        for (;;) {
            const int b0 = peek(k);
            if (b0 < 0) return c;
            k++;
            if (b0 < 0x80) { c.cp = b0; c.b[0] = (uint8_t)b0; c.nb = 1; return c; }
            if (b0 < 0xC2 || b0 > 0xF4) continue;                            // invalid start byte: dropped alone
            const int need = b0 < 0xE0 ? 1 : (b0 < 0xF0 ? 2 : 3);
            int lo = 0x80, hi = 0xBF;                                         // range of the second byte (no overlongs, no surrogates, <= U+10FFFF)
            if (b0 == 0xE0) lo = 0xA0; else if (b0 == 0xED) hi = 0x9F; else if (b0 == 0xF0) lo = 0x90; else if (b0 == 0xF4) hi = 0x8F;
            int cp = need == 1 ? (b0 & 0x1F) : (need == 2 ? (b0 & 0x0F) : (b0 & 0x07));
            c.b[0] = (uint8_t)b0;
            int kk = k, got = 0;
            for (; got < need; got++) {
                const int b = peek(kk);
                if (b < 0 || (got == 0 ? (b < lo || b > hi) : !cont(b))) break;
                cp = (cp << 6) | (b & 0x3F);
                c.b[got + 1] = (uint8_t)b;
                kk++;
            }
            k = kk;                                                           // the bytes read so far are consumed either way
            if (got < need) continue;                                        // broken or truncated sequence: dropped, resume at the offending byte
            c.cp = cp; c.nb = need + 1;
            return c;
        }
    }
};

// Python's str.isspace() per character (what str.strip() removes)
LMRL_HD inline bool py_space(int cp) {
    return (cp >= 9 && cp <= 13) || (cp >= 28 && cp <= 32) || cp == 0x85 || cp == 0xA0 || cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) || cp == 0x2028 ||
           cp == 0x2029 || cp == 0x202F || cp == 0x205F || cp == 0x3000;
}

// ids up to and including the first eos
LMRL_HD inline int cut_at_eos(const int32_t *ids, int n, int eos) {
    if (eos >= 0)
        for (int i = 0; i < n; i++)
            if (ids[i] == eos) return i + 1;
    return n;
}

// generated ids -> the SAN bytes the host path hands the board: decode, `removesuffix('\n') + '\n'` (undone by the strip below), postprocess_move
// (every ' ' removed, then str.strip()), `encode('ascii', errors='replace')[:LMRL_CHESS_ACTION_BYTES - 1]` (VectorChessBoards._strings).
// out: kCAct bytes, NUL padded (a NUL character in the text ends the string, as it does in the fixed-pitch buffer).  -> length
LMRL_HD inline int action_from_tokens(const TokTables &T, const int32_t *ids, int n, char *out) {
    n = cut_at_eos(ids, n, T.eos);
    int first = -1, last = -1, i = 0;
    {
        CharIter it(T, ids, n);
        for (Ch c = it.next(); c.cp >= 0; c = it.next()) {
            if (c.cp == ' ') continue;
            if (!py_space(c.cp)) { if (first < 0) first = i; last = i; }
            i++;
        }
    }
    int len = 0;
    if (first >= 0) {
        CharIter it(T, ids, n);
        i = 0;
        for (Ch c = it.next(); c.cp >= 0 && len < kCAct - 1; c = it.next()) {
            if (c.cp == ' ') continue;
            if (i >= first && i <= last) {
                if (c.cp == 0) break;                       // the board reads a NUL-terminated string (lmrl_chess_agent_step)
                out[len++] = c.cp < 128 ? (char)c.cp : '?';
            }
            i++;
        }
    }
    for (int q = len; q < kCAct; q++) out[q] = 0;
    return len;
}

// prompt ids of a position text: tokenizer.encode(' '.join(fen)) for a tokenizer that encodes that string character by character
LMRL_HD inline int prompt_total(int fen_len) { return fen_len > 0 ? 2 * fen_len - 1 : 0; }
LMRL_HD inline int prompt_token(const int32_t *byte_id, const char *fen_str, int p) {
    return (p & 1) ? byte_id[' '] : byte_id[(uint8_t)fen_str[p >> 1]];
}

LMRL_HD inline int fen_len_of(const char *s) {
    int n = 0;
    while (n < kCFen - 1 && s[n]) n++;
    return n;
}

// the opponent's reply as a generated move (what opponent_half_step does after it has found the move)
LMRL_HD inline void opponent_play(Pos &p, const Move &m, char *san_out, float *reward, int *done) {
    san(p, m, san_out);
    make(p, m);
    *reward = is_checkmate(p) ? -1.f : 0.f;
    *done = is_game_over(p) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------ kernels
// The rules kernels (SAN parsing, move generation, game-over tests) branch per game: 64 games in one wave run one after the other.  A rollout batch
// is a few thousand games on 1024 SIMDs, so the games are spread over the waves — game e runs in lane 0 of every `spread` lanes, still one game
// per lane — which trades idle lanes for games that no longer wait for each other.
static int rules_spread(int n) {
    int s = 64;
    while (s > 1 && (long)n * s > 65536) s >>= 1;
    return s;
}

__global__ void chess_tok_begin_kernel(lmrl_chess_traj tr, Pos *pos, const char *__restrict__ fens, uint8_t *__restrict__ ok, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const char *f = fens + (size_t)e * kCFen;
    const bool good = parse_fen(f, pos[e]);
    ok[e] = good ? 1 : 0;
    const int len = fen_len_of(f);
    char *cur = tr.cur_fen + (size_t)e * kCFen;
    for (int q = 0; q < kCFen; q++) cur[q] = q < len ? f[q] : 0;      // the start position is shown as given (env.py:223-226)
    tr.cur_len[e] = len;
    tr.prev_len[e] = 0;
    tr.keep[e] = 0;
    tr.n_turns[e] = 0;
    tr.ep_reward[e] = 0.f;
    tr.live[e] = good ? 1 : 0;
    tr.gen_active[e] = good ? 1 : 0;
    tr.out_len[e] = 0;
    if (e == 0) tr.flags[0] = 0;
}

// How much of the previous turn's prompt is still in the cache: the K/V rows of the longest common prefix of the previous and the current prompt
// stay (positions [0, keep)), at least one token is forwarded — the rule of the generic policy's prefill (policies.py `_Generator.prefill(reuse=True)`):
// after an illegal move the position, hence the prompt, is unchanged and one token goes through the model; after a move the rows up to the first
// changed square stay.  Sets the session's cache length of every live env to `keep` (0 with reuse off, and on an episode's first turn).
__global__ void chess_tok_prefix_kernel(lmrl_chess_traj tr, const int32_t *__restrict__ byte_id, int max_input_length, int reuse, int32_t *__restrict__ len_d,
                                        int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    int keep = 0;
    if (tr.live[e]) {
        const char *cur = tr.cur_fen + (size_t)e * kCFen, *prev = tr.prev_fen + (size_t)e * kCFen;
        const int total = prompt_total(tr.cur_len[e]), ptotal = prompt_total(tr.prev_len[e]);
        const int start = total > max_input_length ? total - max_input_length : 0, pstart = ptotal > max_input_length ? ptotal - max_input_length : 0;
        const int len = total - start, plen = ptotal - pstart;
        const int lim = min(plen, len - 1);
        if (reuse)
            while (keep < lim && prompt_token(byte_id, cur, start + keep) == prompt_token(byte_id, prev, pstart + keep)) keep++;
        for (int q = 0; q < kCFen; q++) tr.prev_fen[(size_t)e * kCFen + q] = cur[q];
        tr.prev_len[e] = tr.cur_len[e];
    }
    tr.keep[e] = keep;
    len_d[e] = keep;
}

__global__ void chess_tok_prompt_kernel(lmrl_chess_traj tr, const int32_t *__restrict__ byte_id, int j, int chunk, int max_input_length, int budget,
                                        int32_t *__restrict__ chunk_tok, int32_t *__restrict__ chunk_cnt, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * chunk) return;
    const int e = i / chunk, k = i - e * chunk;
    int total = tr.live[e] ? prompt_total(tr.cur_len[e]) : 0;
    const int keep = tr.keep[e];
    const int start = (total > max_input_length ? total - max_input_length : 0) + keep;  // Truncation.LEFT (ppo/gpt2/interface.py:519-524)
    int len = total - start;
    if (len + keep > budget) {                                                           // longer than the chunks the caller scheduled
        if (k == 0 && j == 0) atomicOr(tr.flags, 1);
        len = max(0, budget - keep);
    }
    const int p = j * chunk + k;
    chunk_tok[i] = p < len ? prompt_token(byte_id, tr.cur_fen + (size_t)e * kCFen, start + p) : 0;
    if (k == 0) chunk_cnt[e] = max(0, min(chunk, len - j * chunk));
}

__global__ void chess_tok_action_kernel(lmrl_chess_traj tr, Pos *pos, TokTables T, int max_new, int max_turns, int spread, int n) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g % spread) return;
    const int e = g / spread;
    if (e >= n) return;
    char *u = tr.uci + (size_t)e * 8;
    if (!tr.live[e]) {
        tr.res[e] = 255;
        u[0] = 0;
        return;
    }
    const int t = tr.n_turns[e];
    int len = tr.out_len[e];
    len = len < 0 ? 0 : (len > max_new ? max_new : len);
    const int32_t *ids = tr.out_tok + (size_t)e * max_new;
    for (int k = 0; k < len; k++) tr.gen[((size_t)e * max_turns + t) * max_new + k] = ids[k];
    tr.gen_len[(size_t)e * max_turns + t] = len;
    char a[kCAct];
    const int al = action_from_tokens(T, ids, len, a);
    for (int q = 0; q < kCAct; q++) {
        tr.act[(size_t)e * kCAct + q] = a[q];
        tr.action[((size_t)e * max_turns + t) * kCAct + q] = a[q];
    }
    float r; int d;
    char um[8];
    const int res = agent_half_step(pos[e], a, al, &r, &d, um);
    tr.res[e] = (uint8_t)res; tr.rew[e] = r; tr.dn[e] = (uint8_t)d;
    bool z = res != LMRL_CHESS_MOVED;                // only a game that waits for a reply hands its move down
    for (int q = 0; q < 8; q++) { if (!z && !um[q]) z = true; u[q] = z ? 0 : um[q]; }
    for (int q = 0; q < kCAct; q++) tr.cur_san[(size_t)e * kCAct + q] = 0;
    for (int q = 0; q < 8; q++) tr.cur_reply[(size_t)e * 8 + q] = 0;
    tr.reply_ok[e] = 1;
}

// the device opponent: one of the position's legal moves, by a counter-based draw or by an injected index table
__global__ void chess_tok_opponent_kernel(lmrl_chess_traj tr, Pos *pos, uint32_t seed_lo, uint32_t seed_hi, const uint32_t *__restrict__ epoch,
                                          const int32_t *__restrict__ reply_idx, int reply_turns, int spread, int n) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g % spread) return;
    const int e = g / spread;
    if (e >= n || tr.res[e] != LMRL_CHESS_MOVED) return;
    Move mv[kMaxMoves];
    const int count = gen_legal(pos[e], mv);
    if (count <= 0) { tr.reply_ok[e] = 0; return; }            // (a MOVED result means the game is not over: there is a legal move)
    const int t = tr.n_turns[e];
    int idx;
    if (reply_idx) {
        const int v = reply_idx[(size_t)(t < reply_turns ? t : reply_turns - 1) * n + e];
        idx = ((v % count) + count) % count;
    } else {
        const uint32_t w = chess_philox_word((uint32_t)e, (uint32_t)t, LMRL_CHESS_REPLY_STREAM, epoch ? *epoch : 0u, seed_lo, seed_hi);
        idx = (int)(((uint64_t)w * (uint64_t)count) >> 32);
    }
    uci(mv[idx], tr.cur_reply + (size_t)e * 8);
    float r; int d;
    opponent_play(pos[e], mv[idx], tr.cur_san + (size_t)e * kCAct, &r, &d);
    tr.rew[e] = r; tr.dn[e] = (uint8_t)d;
}

// the host opponent: tr.cur_reply [n][8] came up from the engine pool
__global__ void chess_tok_opponent_host_kernel(lmrl_chess_traj tr, Pos *pos, int spread, int n) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g % spread) return;
    const int e = g / spread;
    if (e >= n || tr.res[e] != LMRL_CHESS_MOVED) return;
    const char *u = tr.cur_reply + (size_t)e * 8;
    int len = 0;
    while (len < 7 && u[len]) len++;
    float r = 0.f; int d = 0;
    const bool ok = opponent_half_step(pos[e], u, len, tr.cur_san + (size_t)e * kCAct, &r, &d);
    tr.reply_ok[e] = ok ? 1 : 0;
    if (ok) { tr.rew[e] = r; tr.dn[e] = (uint8_t)d; }
}

__global__ void chess_tok_result_kernel(lmrl_chess_traj tr, const Pos *pos, int max_moves, int max_turns, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    tr.out_len[e] = 0;
    if (!tr.live[e] || tr.res[e] == 255) { tr.gen_active[e] = 0; return; }
    const int t = tr.n_turns[e];
    const size_t row = (size_t)e * max_turns + t;
    char *cur = tr.cur_fen + (size_t)e * kCFen;
    for (int q = 0; q < kCFen; q++) tr.fen[row * kCFen + q] = cur[q];
    char f[kCFen];
    int len = fen(pos[e], f);
    len = len < kCFen - 1 ? len : kCFen - 1;
    for (int q = 0; q < kCFen; q++) cur[q] = q < len ? f[q] : 0;
    tr.cur_len[e] = len;
    for (int q = 0; q < kCAct; q++) tr.opp_san[row * kCAct + q] = tr.cur_san[(size_t)e * kCAct + q];
    for (int q = 0; q < 8; q++) tr.reply[row * 8 + q] = tr.cur_reply[(size_t)e * 8 + q];
    const float r = tr.rew[e];
    const bool done = tr.dn[e] || t + 1 > max_moves;                     // FenChessHistoryEnv: num_moves_made > max_moves (env.py:228-236)
    tr.result[row] = tr.res[e];
    tr.reward[row] = r;
    tr.done[row] = done ? 1 : 0;
    tr.ep_reward[e] += r;
    tr.n_turns[e] = t + 1;
    const bool live = !done && t + 1 < max_turns;                         // record full: the episode is cut here (the host sizes T = max_moves + 1)
    tr.live[e] = live ? 1 : 0;
    tr.gen_active[e] = live ? 1 : 0;
}

// ---- the finished episodes as PPO records: one token trajectory per transition — the prompt ids of the observation ++ the action ids, the turn's
// reward on the action's last token — chained per episode (chess/ppo/train_ppo_gpt2_online.py:293-314: TextTrajectory(post_action_history, [0, r],
// done) + TokenTrajectory.from_text_trajectory).  The action ids re-encode the action TEXT `decode(ids).removesuffix('\n') + '\n'`: for byte ids
// the UTF-8 bytes of the decoded characters, otherwise the generated ids minus special ids; a newline id is appended when the text has none at
// its end.  One wave per env (rows off[e] + t); lane 0 walks the action, the wave copies the prompt.
__global__ __launch_bounds__(256) void chess_ppo_records_kernel(lmrl_chess_traj tr, TokTables T, int max_new, int max_turns, int n, const int32_t *__restrict__ off,
                                                                int newline_tok, int cap, int32_t *__restrict__ tokens, uint8_t *__restrict__ is_action,
                                                                float *__restrict__ reward, int32_t *__restrict__ n_tok, int32_t *__restrict__ chain,
                                                                int32_t *__restrict__ pos, uint8_t *__restrict__ last, uint8_t *__restrict__ done,
                                                                int32_t *__restrict__ chain_total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + wave;
    if (e >= n) return;
    const int nt = tr.n_turns[e];
    int offset = 0;
    for (int t = 0; t < nt; t++) {
        const size_t row = (size_t)off[e] + t, rec = (size_t)e * max_turns + t;
        const char *f = tr.fen + rec * kCFen;
        const int ol = min(prompt_total(fen_len_of(f)), cap);
        for (int k = lane; k < ol; k += 64) {
            tokens[row * cap + k] = prompt_token(T.byte_id, f, k);
            is_action[row * cap + k] = 0;
            reward[row * cap + k] = 0.f;
        }
        const int32_t *ids = tr.gen + rec * max_new;
        const int gl = cut_at_eos(ids, tr.gen_len[rec], T.eos);
        int na = 0, last_cp = -1;
        if (T.byte_ids) {
            CharIter it(T, ids, gl);
            for (Ch c = it.next(); c.cp >= 0; c = it.next()) {
                if (lane == 0)
                    for (int b = 0; b < c.nb; b++)
                        if (ol + na + b < cap) tokens[row * cap + ol + na + b] = c.b[b];
                na += c.nb;
                last_cp = c.cp;
            }
        } else {
            for (int k = 0; k < gl; k++) {
                const int tok = ids[k];
                const int bl = (tok >= 0 && tok < T.vocab) ? T.tok_blen[tok] : 255;
                if (bl == 0) continue;
                if (lane == 0 && ol + na < cap) tokens[row * cap + ol + na] = tok;
                last_cp = bl == 255 ? -1 : T.tok_bytes[(size_t)tok * kCTokBytes + bl - 1];
                na++;
            }
        }
        if (last_cp != '\n') {
            if (lane == 0 && ol + na < cap) tokens[row * cap + ol + na] = newline_tok;
            na++;
        }
        const int total = min(ol + na, cap);
        for (int k = ol + lane; k < total; k += 64) {
            is_action[row * cap + k] = 1;
            reward[row * cap + k] = k == total - 1 ? tr.reward[rec] : 0.f;
        }
        if (lane == 0) {
            n_tok[row] = total;
            chain[row] = e;
            pos[row] = offset;
            last[row] = t == nt - 1;
        }
        offset += total > 0 ? total - 1 : 0;
    }
    if (lane == 0) {
        done[e] = nt > 0 ? tr.done[(size_t)e * max_turns + nt - 1] : 0;
        chain_total[e] = offset;
    }
}

static TokTables tables_of(const lmrl_chess_tok_ctx *c, bool host) {
    TokTables T;
    T.byte_id = host ? c->byte_id_h : c->byte_id_d;
    T.tok_bytes = host ? c->tok_bytes_h : c->tok_bytes_d;
    T.tok_blen = host ? c->tok_blen_h : c->tok_blen_d;
    T.vocab = c->vocab; T.byte_ids = c->byte_ids; T.eos = c->eos;
    return T;
}

}  // namespace lmrl

using namespace lmrl;

extern "C" {

lmrl_chess_tok_ctx *lmrl_chess_tok_create(const int32_t *byte_id, const uint8_t *tok_bytes, const uint8_t *tok_blen, int vocab, int byte_ids, int eos_token,
                                          int max_new_tokens, int max_turns, int host_only) {
    if (!byte_id || !tok_bytes || !tok_blen || vocab <= 0 || max_new_tokens <= 0 || max_turns <= 0 || max_turns >= 4096) {
        set_error("lmrl_chess_tok_create: bad argument");
        return nullptr;
    }
    for (int i = 0; i < 256; i++)
        if (byte_id[i] >= vocab) { set_error("lmrl_chess_tok_create: byte id outside the vocabulary"); return nullptr; }
    auto *c = new lmrl_chess_tok_ctx();
    c->vocab = vocab; c->byte_ids = byte_ids ? 1 : 0; c->eos = eos_token; c->max_new = max_new_tokens; c->max_turns = max_turns;
    memcpy(c->byte_id_h, byte_id, sizeof(c->byte_id_h));
    c->tok_bytes_h = new uint8_t[(size_t)vocab * kCTokBytes];
    c->tok_blen_h = new uint8_t[vocab];
    memcpy(c->tok_bytes_h, tok_bytes, (size_t)vocab * kCTokBytes);
    memcpy(c->tok_blen_h, tok_blen, vocab);
    if (!host_only) {
        bool ok = hipMalloc((void **)&c->byte_id_d, sizeof(c->byte_id_h)) == hipSuccess &&
                  hipMalloc((void **)&c->tok_bytes_d, (size_t)vocab * kCTokBytes) == hipSuccess && hipMalloc((void **)&c->tok_blen_d, vocab) == hipSuccess;
        ok = ok && hipMemcpy(c->byte_id_d, byte_id, sizeof(c->byte_id_h), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(c->tok_bytes_d, tok_bytes, (size_t)vocab * kCTokBytes, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(c->tok_blen_d, tok_blen, vocab, hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) {
            set_error("lmrl_chess_tok_create: device allocation failed");
            lmrl_chess_tok_destroy(c);
            return nullptr;
        }
    }
    return c;
}

void lmrl_chess_tok_destroy(lmrl_chess_tok_ctx *c) {
    if (!c) return;
    if (c->byte_id_d) (void)hipFree(c->byte_id_d);
    if (c->tok_bytes_d) (void)hipFree(c->tok_bytes_d);
    if (c->tok_blen_d) (void)hipFree(c->tok_blen_d);
    delete[] c->tok_bytes_h;
    delete[] c->tok_blen_h;
    delete c;
}

#define CHESS_TOK_DEVICE(c, what) LMRL_REQUIRE((c) && (c)->byte_id_d, what ": needs a context created with host_only = 0")

int lmrl_chess_tok_begin(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, void *pos_d, const char *fens_d, uint8_t *ok_d, int n, void *stream) {
    CHESS_TOK_DEVICE(c, "lmrl_chess_tok_begin");
    LMRL_REQUIRE(tr && pos_d && fens_d && ok_d && n > 0, "lmrl_chess_tok_begin: bad argument");
    hipLaunchKernelGGL(chess_tok_begin_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, as_stream(stream), *tr, (Pos *)pos_d, fens_d, ok_d, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_chess_tok_prefix(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, int max_input_length, int reuse, int32_t *len_d, int n, void *stream) {
    CHESS_TOK_DEVICE(c, "lmrl_chess_tok_prefix");
    LMRL_REQUIRE(tr && len_d && n > 0 && max_input_length > 0, "lmrl_chess_tok_prefix: bad argument");
    hipLaunchKernelGGL(chess_tok_prefix_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, as_stream(stream), *tr, c->byte_id_d, max_input_length, reuse, len_d, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_chess_tok_prompt(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, int j, int chunk, int max_input_length, int n_chunks, int32_t *chunk_tok_d,
                          int32_t *chunk_cnt_d, int n, void *stream) {
    CHESS_TOK_DEVICE(c, "lmrl_chess_tok_prompt");
    LMRL_REQUIRE(tr && chunk_tok_d && chunk_cnt_d && n > 0 && chunk > 0 && j >= 0 && j < n_chunks && max_input_length > 0, "lmrl_chess_tok_prompt: bad argument");
    hipLaunchKernelGGL(chess_tok_prompt_kernel, dim3(ceil_div((long)n * chunk, 256)), dim3(256), 0, as_stream(stream), *tr, c->byte_id_d, j, chunk,
                       max_input_length, n_chunks * chunk, chunk_tok_d, chunk_cnt_d, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_chess_tok_action(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, void *pos_d, int n, void *stream) {
    CHESS_TOK_DEVICE(c, "lmrl_chess_tok_action");
    LMRL_REQUIRE(tr && pos_d && n > 0, "lmrl_chess_tok_action: bad argument");
    const int spread = rules_spread(n);
    hipLaunchKernelGGL(chess_tok_action_kernel, dim3(ceil_div((long)n * spread, 64)), dim3(64), 0, as_stream(stream), *tr, (Pos *)pos_d, tables_of(c, false),
                       c->max_new, c->max_turns, spread, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_chess_tok_opponent(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, void *pos_d, uint64_t seed, const uint32_t *epoch_d, const int32_t *reply_idx_d,
                            int reply_turns, int n, void *stream) {
    CHESS_TOK_DEVICE(c, "lmrl_chess_tok_opponent");
    LMRL_REQUIRE(tr && pos_d && n > 0 && (!reply_idx_d || reply_turns > 0), "lmrl_chess_tok_opponent: bad argument");
    const int spread = rules_spread(n);
    hipLaunchKernelGGL(chess_tok_opponent_kernel, dim3(ceil_div((long)n * spread, 64)), dim3(64), 0, as_stream(stream), *tr, (Pos *)pos_d, (uint32_t)seed,
                       (uint32_t)(seed >> 32), epoch_d, reply_idx_d, reply_turns, spread, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_chess_tok_opponent_host(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, void *pos_d, int n, void *stream) {
    CHESS_TOK_DEVICE(c, "lmrl_chess_tok_opponent_host");
    LMRL_REQUIRE(tr && pos_d && n > 0, "lmrl_chess_tok_opponent_host: bad argument");
    const int spread = rules_spread(n);
    hipLaunchKernelGGL(chess_tok_opponent_host_kernel, dim3(ceil_div((long)n * spread, 64)), dim3(64), 0, as_stream(stream), *tr, (Pos *)pos_d, spread, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_chess_tok_result(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, const void *pos_d, int max_moves, int n, void *stream) {
    CHESS_TOK_DEVICE(c, "lmrl_chess_tok_result");
    LMRL_REQUIRE(tr && pos_d && n > 0 && max_moves >= 0, "lmrl_chess_tok_result: bad argument");
    hipLaunchKernelGGL(chess_tok_result_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, as_stream(stream), *tr, (const Pos *)pos_d, max_moves, c->max_turns, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_chess_tok_ppo_records(lmrl_chess_tok_ctx *c, const lmrl_chess_traj *tr, int n, const int32_t *off_d, int newline_tok, int cap, int32_t *tokens_d,
                               uint8_t *is_action_d, float *reward_d, int32_t *n_tok_d, int32_t *chain_d, int32_t *pos_d, uint8_t *last_d, uint8_t *done_d,
                               int32_t *chain_total_d, void *stream) {
    CHESS_TOK_DEVICE(c, "lmrl_chess_tok_ppo_records");
    LMRL_REQUIRE(tr && n > 0 && off_d && cap > 0 && tokens_d && is_action_d && reward_d && n_tok_d && chain_d && pos_d && last_d && done_d && chain_total_d,
                 "lmrl_chess_tok_ppo_records: bad argument");
    hipLaunchKernelGGL(chess_ppo_records_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, as_stream(stream), *tr, tables_of(c, false), c->max_new, c->max_turns, n, off_d,
                       newline_tok, cap, tokens_d, is_action_d, reward_d, n_tok_d, chain_d, pos_d, last_d, done_d, chain_total_d);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

// ---- host faces of the string work (no GPU needed): the same LMRL_HD functions on host memory
int lmrl_chess_host_prompt_tokens(const lmrl_chess_tok_ctx *c, const char *fen_str, int max_input_length, int32_t *out, int out_cap) {
    if (!c || !fen_str || !out || max_input_length <= 0) return -1;
    char f[kCFen];
    int len = 0;
    for (; len < kCFen - 1 && fen_str[len]; len++) f[len] = fen_str[len];
    f[len] = 0;
    const int total = prompt_total(len);
    const int start = total > max_input_length ? total - max_input_length : 0;
    if (total - start > out_cap) return -1;
    for (int p = start; p < total; p++) out[p - start] = prompt_token(c->byte_id_h, f, p);
    return total - start;
}

int lmrl_chess_host_action_from_tokens(const lmrl_chess_tok_ctx *c, const int32_t *ids, int n, char *out) {
    if (!c || (!ids && n > 0) || n < 0 || !out) return -1;
    return action_from_tokens(tables_of(c, true), ids, n, out);
}

uint32_t lmrl_chess_host_reply_word(uint64_t seed, uint32_t epoch, uint32_t turn, uint32_t env) {
    return chess_philox_word(env, turn, LMRL_CHESS_REPLY_STREAM, epoch, (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // extern "C"
