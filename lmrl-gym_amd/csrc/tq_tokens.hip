// tq_tokens.hip — on-device token <-> game bookkeeping for lock-step Twenty Questions rollouts (twenty_questions/ppo/train_ppo.py with
// twenty_questions/env/{env,data,oracle}.py), the only env of the package with TWO models in the loop.
//
// The host path per turn: decode the guesser's ids, `out_str_process`, build B oracle prompt strings, tokenise them, run the oracle policy, regex
// the B answers, `is_done` in Python, hand text back to the guesser, which tokenises the whole history again.  Here a turn is
//   guesser decode | question (ids -> text -> canonical ids, strip, oracle prompt, kept prefixes) | oracle prefill + <= 4 greedy steps |
//   answer (ids -> "Yes." / "No.") | judge (guessed, reward, done, record) | guesser chunk (the question's unforwarded tail + the answer)
// with nothing leaving HBM.  The text rules are tq_core.h (plain functions, shared with the host faces at the bottom); these kernels are integer
// and byte work, one env per lane (a rollout batch is <= a few thousand envs; the two transformers are the turn's cost), no LDS.
// In scope: tokenizers whose ids are the text's UTF-8 bytes (the caller probes it), histories that fit without truncation.
#include "../../include/lmrl_amd.h"
#include "common.h"
#include "mt19937.h"
#include "tq_core.h"
#include <string.h>
#include <vector>

using lmrl_tq::TqTables;

struct lmrl_tq_ctx {
    // host copies (the host faces) and device copies of the tables
    std::vector<uint8_t> bytes_h, tok_blen_h, invalid_h;
    std::vector<int32_t> str_off_h, spell_off_h, word_off_h, prefix_h, prefix_len_h, suffix_h, init_h, yes_h, no_h;
    uint8_t *bytes_d = nullptr, *tok_blen_d = nullptr, *invalid_d = nullptr;
    int32_t *str_off_d = nullptr, *spell_off_d = nullptr, *word_off_d = nullptr, *prefix_d = nullptr, *prefix_len_d = nullptr, *suffix_d = nullptr,
            *init_d = nullptr, *yes_d = nullptr, *no_d = nullptr;
    int n_det = 0, n_func = 0, n_generic = 0, n_words = 0, prefix_cap = 0, vocab = 0, eos = -1, oracle_eos = -1;
    int G = 0, OG = 0, T = 0, Q = 0;
    bool device = false;
};

namespace lmrl {

static TqTables tables_of(const lmrl_tq_ctx *c, bool host, bool oracle) {
    TqTables t;
    t.bytes = host ? c->bytes_h.data() : c->bytes_d;
    t.str_off = host ? c->str_off_h.data() : c->str_off_d;
    t.spell_off = host ? c->spell_off_h.data() : c->spell_off_d;
    t.word_off = host ? c->word_off_h.data() : c->word_off_d;
    t.n_det = c->n_det; t.n_func = c->n_func; t.n_generic = c->n_generic; t.n_words = c->n_words;
    t.tok_blen = host ? c->tok_blen_h.data() : c->tok_blen_d;
    t.vocab = c->vocab; t.eos = oracle ? c->oracle_eos : c->eos;
    t.invalid_q = host ? c->invalid_h.data() : c->invalid_d;
    t.invalid_q_len = (int)c->invalid_h.size();
    return t;
}

struct TqDims {                 // per-context sizes and the small id tables every kernel may need
    const int32_t *prefix, *prefix_len, *suffix, *init, *yes, *no;
    int prefix_cap, suffix_len, init_len, yes_len, no_len, G, OG, T, Q;
};

static TqDims dims_of(const lmrl_tq_ctx *c) {
    TqDims d;
    d.prefix = c->prefix_d; d.prefix_len = c->prefix_len_d; d.suffix = c->suffix_d; d.init = c->init_d; d.yes = c->yes_d; d.no = c->no_d;
    d.prefix_cap = c->prefix_cap; d.suffix_len = (int)c->suffix_h.size(); d.init_len = (int)c->init_h.size();
    d.yes_len = (int)c->yes_h.size(); d.no_len = (int)c->no_h.size();
    d.G = c->G; d.OG = c->OG; d.T = c->T; d.Q = c->Q;
    return d;
}

// prefix[word] ++ question ++ suffix -> out (cap ids).  -> length, or -1 when it does not fit
LMRL_HD int oracle_prompt(const int32_t *prefix, int plen, const uint8_t *q, int qn, const int32_t *suffix, int slen, int32_t *out, int cap) {
    if (plen + qn + slen > cap) return -1;
    int k = 0;
    for (int i = 0; i < plen; i++) out[k++] = prefix[i];
    for (int i = 0; i < qn; i++) out[k++] = q[i];
    for (int i = 0; i < slen; i++) out[k++] = suffix[i];
    return k;
}

// episode start: the hidden word (deterministic mode: seed % n_words; else the first _randbelow(n_words) draw of random.Random(seed), drawn by the
// caller through lmrl_mt_seed + lmrl_mt_randbelow), the history = INITIAL_STR (to be forwarded: feed range), records and counters cleared
__global__ void tq_reset_kernel(lmrl_tq_traj tr, TqDims D, const uint64_t *__restrict__ seeds, const uint8_t *__restrict__ deterministic,
                                const uint32_t *__restrict__ draws, int n_words, int n_live, int32_t *__restrict__ len_g, int32_t *__restrict__ len_o, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) tr.flags[0] = 0;
    if (e >= n) return;
    tr.word[e] = (deterministic && deterministic[e]) ? (int)(seeds[e] % (uint64_t)n_words) : (int)(draws[e] % (uint32_t)n_words);
    const bool live = e < n_live;
    tr.n_turns[e] = 0; tr.ep_reward[e] = 0.f;
    tr.live[e] = live ? 1 : 0; tr.gen_active[e] = live ? 1 : 0;
    tr.out_len[e] = 0; tr.o_out_len[e] = 0; tr.o_active[e] = 0; tr.ans[e] = 0;
    for (int t = 0; t < D.T; t++) {
        const size_t r = (size_t)e * D.T + t;
        tr.gen_len[r] = 0; tr.q_len[r] = 0; tr.q_off[r] = 0; tr.ogen_len[r] = 0; tr.answer[r] = 0; tr.reward[r] = 0.f; tr.done[r] = 0; tr.flag[r] = 0;
    }
    int32_t *hist = tr.hist + (size_t)e * tr.hcap;
    const int il = min(D.init_len, tr.hcap);
    for (int k = 0; k < il; k++) hist[k] = D.init[k];
    tr.hist_len[e] = il;
    tr.feed_start[e] = 0;
    tr.feed_len[e] = live ? il : 0;
    tr.o_len[e] = 0; tr.o_prev_len[e] = 0; tr.o_keep[e] = 0;
    tr.strip_b[e] = 0; tr.strip_e[e] = 0;
    len_g[e] = 0;
    len_o[e] = 0;
}

// after the guesser's decode steps.  Live env: ids -> the question text (record row of this turn) -> its canonical ids onto the history; the K/V
// rows of the generated ids that went through the model (all but the last: lmrl_gen_accept) stay as far as they ARE the canonical ids — the
// guesser's cache is cut back to history + that common prefix (keep_generated == 0: to the history alone, the generic policy's prefill) and the
// rest is this turn's feed.  Every env: the oracle prompt (finished envs ask INVALID_QUESTION about their own word) and how much of the oracle's
// cache survives: the longest common prefix of the previous and this prompt, at least one token forwarded (`GPT2PPOPolicy(reuse_kv=True)`).
__global__ void tq_question_kernel(lmrl_tq_traj tr, TqTables T, TqDims D, int keep_generated, int32_t *__restrict__ len_g, int32_t *__restrict__ len_o, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int w = tr.word[e];
    int32_t *op = tr.o_prompt + (size_t)e * tr.pcap;
    int ol;
    if (tr.live[e]) {
        const int t = tr.n_turns[e];
        const size_t r = (size_t)e * D.T + t;
        int gl = tr.out_len[e];
        gl = gl < 0 ? 0 : (gl > D.G ? D.G : gl);
        const int32_t *ids = tr.out_tok + (size_t)e * D.G;
        for (int k = 0; k < gl; k++) tr.gen[r * D.G + k] = ids[k];
        tr.gen_len[r] = gl;
        uint8_t *q = tr.q_text + r * D.Q;
        int sb, se;
        const int ql = lmrl_tq::question_from_ids(T, ids, gl, q, D.Q, &sb, &se);
        tr.q_len[r] = ql;
        tr.strip_b[e] = sb; tr.strip_e[e] = se;
        const int base = tr.hist_len[e];
        int32_t *hist = tr.hist + (size_t)e * tr.hcap;
        if (base + ql + max(D.yes_len, D.no_len) > tr.hcap) {           // (the constructor sizes the history for T full turns: never)
            atomicOr(tr.flags, 2);
            tr.live[e] = 0; tr.gen_active[e] = 0; tr.feed_len[e] = 0;
        } else {
            for (int k = 0; k < ql; k++) hist[base + k] = q[k];
            tr.q_off[r] = base;
            const int fwd = gl > 0 ? gl - 1 : 0;
            int lcp = 0;
            if (keep_generated)
                while (lcp < fwd && lcp < ql && ids[lcp] == (int32_t)q[lcp]) lcp++;
            len_g[e] = base + lcp;
            tr.feed_start[e] = base + lcp;
            tr.hist_len[e] = base + ql;
        }
        ol = oracle_prompt(D.prefix + (size_t)w * D.prefix_cap, D.prefix_len[w], q + sb, se - sb, D.suffix, D.suffix_len, op, tr.pcap);
    } else {
        tr.feed_len[e] = 0;
        ol = oracle_prompt(D.prefix + (size_t)w * D.prefix_cap, D.prefix_len[w], T.invalid_q, T.invalid_q_len, D.suffix, D.suffix_len, op, tr.pcap);
    }
    if (ol < 0) { atomicOr(tr.flags, 4); ol = 0; }
    int32_t *prev = tr.o_prev + (size_t)e * tr.pcap;
    const int lim = min(tr.o_prev_len[e], ol - 1);
    int keep = 0;
    while (keep < lim && prev[keep] == op[keep]) keep++;
    for (int k = keep; k < ol; k++) prev[k] = op[k];
    tr.o_prev_len[e] = ol;
    tr.o_len[e] = ol;
    tr.o_keep[e] = keep;
    len_o[e] = keep;
    tr.o_out_len[e] = 0;
    tr.o_active[e] = ol > 0 ? 1 : 0;
}

// chunk j of the oracle prompts behind their kept prefix / of the guesser's feed range of the history: tokens [n][chunk], counts [n]
__global__ void tq_chunk_kernel(const int32_t *__restrict__ src, int pitch, const int32_t *__restrict__ start, const int32_t *__restrict__ len_or_end,
                                int end_form, int j, int chunk, int budget, int32_t *__restrict__ flags, int flag_bit, int32_t *__restrict__ chunk_tok,
                                int32_t *__restrict__ chunk_cnt, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * chunk) return;
    const int e = i / chunk, k = i - e * chunk;
    const int s = start[e];
    int len = end_form ? len_or_end[e] - s : len_or_end[e];
    len = len < 0 ? 0 : len;
    if (len > budget) {                                                  // more than the chunks the caller scheduled
        if (k == 0 && j == 0) atomicOr(flags, flag_bit);
        len = budget;
    }
    const int p = j * chunk + k;
    chunk_tok[i] = p < len ? src[(size_t)e * pitch + s + p] : 0;
    if (k == 0) chunk_cnt[e] = max(0, min(chunk, len - j * chunk));
}

// after the oracle's decode steps: its ids -> "Yes." / "No." (`answers_from_outputs`), or the injected table; the answer's ids join the history
// and the guesser's feed
__global__ void tq_answer_kernel(lmrl_tq_traj tr, TqTables T, TqDims D, const int8_t *__restrict__ scripted, int script_turns, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || !tr.live[e]) return;
    const int t = tr.n_turns[e];
    const size_t r = (size_t)e * D.T + t;
    int ol = tr.o_out_len[e];
    ol = ol < 0 ? 0 : (ol > D.OG ? D.OG : ol);
    const int32_t *ids = tr.o_out_tok + (size_t)e * D.OG;
    for (int k = 0; k < ol; k++) tr.ogen[r * D.OG + k] = ids[k];
    tr.ogen_len[r] = ol;
    int code = -1;
    if (scripted) code = scripted[(size_t)e * script_turns + (t < script_turns ? t : script_turns - 1)];
    if (code < 0) {
        uint8_t text[16];
        static_assert(LMRL_TQ_ORACLE_MAX_NEW <= 16, "scratch of the answer text");
        code = lmrl_tq::answer_from_ids(T, tr.q_text + r * D.Q + tr.strip_b[e], tr.strip_e[e] - tr.strip_b[e], ids, ol, text, 16);
    }
    code = code ? 1 : 0;
    tr.ans[e] = (uint8_t)code;
    tr.answer[r] = (uint8_t)code;
    const int32_t *a = code ? D.yes : D.no;
    const int al = code ? D.yes_len : D.no_len;
    int32_t *hist = tr.hist + (size_t)e * tr.hcap;
    const int base = tr.hist_len[e];                                     // (room for the answer was checked with the question)
    for (int k = 0; k < al; k++) hist[base + k] = a[k];
    tr.hist_len[e] = base + al;
    tr.feed_len[e] = base + al - tr.feed_start[e];
}

// guessed / reward / done of `_verdicts`, the record, counters, live flags of the next turn.  An affirmed question the device cannot judge exactly
// (a byte >= 0x80; device_judge == 0: every one) is NOT guessed here: the game goes on and the turn is flagged for the host.
__global__ void tq_judge_kernel(lmrl_tq_traj tr, TqTables T, TqDims D, int device_judge, int max_conversation_length, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    tr.out_len[e] = 0;
    if (!tr.live[e]) { tr.gen_active[e] = 0; return; }
    const int t = tr.n_turns[e];
    const size_t r = (size_t)e * D.T + t;
    bool guessed = false, flagged = false;
    if (tr.ans[e]) {
        int judgeable = 0;
        if (device_judge) guessed = lmrl_tq::is_done(T, tr.word[e], tr.q_text + r * D.Q + tr.strip_b[e], tr.strip_e[e] - tr.strip_b[e], &judgeable);
        flagged = !judgeable;
    }
    const bool done = guessed || t + 1 >= max_conversation_length;
    const float rew = guessed ? 0.f : -1.f;
    tr.reward[r] = rew;
    tr.done[r] = done ? 1 : 0;
    tr.flag[r] = flagged ? 1 : 0;
    tr.ep_reward[e] += rew;
    tr.n_turns[e] = t + 1;
    const bool live = !done && t + 1 < D.T;
    tr.live[e] = live ? 1 : 0;
    tr.gen_active[e] = live ? 1 : 0;
    if (!live) tr.feed_len[e] = 0;                                       // a finished game's history is not forwarded any more
}

// One token trajectory per episode: the whole history, the questions' tokens as actions, each turn's reward on its question's last token
// (twenty_questions/ppo/train_ppo.py:322-352 + TokenTrajectory.from_text_trajectory).  One wave per env.
__global__ __launch_bounds__(256) void tq_ppo_records_kernel(lmrl_tq_traj tr, TqDims D, int n, int cap, int32_t *__restrict__ tokens, uint8_t *__restrict__ is_action,
                                                             float *__restrict__ reward, int32_t *__restrict__ n_tok, uint8_t *__restrict__ done) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + wave;
    if (e >= n) return;
    const int nt = min(tr.n_turns[e], D.T);
    int total = min(D.init_len, tr.hcap);
    if (nt > 0) {
        const size_t r = (size_t)e * D.T + nt - 1;
        total = tr.q_off[r] + tr.q_len[r] + (tr.answer[r] ? D.yes_len : D.no_len);
    }
    total = min(min(total, cap), tr.hcap);
    const int32_t *hist = tr.hist + (size_t)e * tr.hcap;
    for (int k = lane; k < total; k += 64) {
        uint8_t ia = 0;
        float rw = 0.f;
        for (int t = 0; t < nt; t++) {
            const size_t r = (size_t)e * D.T + t;
            const int a = tr.q_off[r], b = a + tr.q_len[r];
            if (k >= a && k < b) { ia = 1; if (k == b - 1) rw = tr.reward[r]; }
        }
        tokens[(size_t)e * cap + k] = hist[k];
        is_action[(size_t)e * cap + k] = ia;
        reward[(size_t)e * cap + k] = rw;
    }
    if (lane == 0) {
        n_tok[e] = total;
        done[e] = nt > 0 ? tr.done[(size_t)e * D.T + nt - 1] : 0;
    }
}

}  // namespace lmrl

using namespace lmrl;

extern "C" {

lmrl_tq_ctx *lmrl_tq_create(const lmrl_tq_tables *t, int host_only) {
    if (!t || !t->bytes || !t->str_off || !t->spell_off || !t->word_off || !t->tok_blen || !t->prefix || !t->prefix_len || !t->suffix || !t->invalid_question ||
        !t->initial || !t->yes || !t->no || t->n_words <= 0 || t->n_strings < 0 || t->n_spellings < 0 || t->vocab < 256 || t->prefix_cap <= 0 ||
        t->suffix_len < 0 || t->invalid_len <= 0 || t->initial_len <= 0 || t->yes_len <= 0 || t->no_len <= 0 || t->max_new_tokens <= 0 ||
        t->oracle_max_new_tokens <= 0 || t->oracle_max_new_tokens > LMRL_TQ_ORACLE_MAX_NEW || t->max_turns <= 0 || t->n_det < 0 || t->n_func < 0 ||
        t->n_generic < 0 || t->n_det + t->n_func + t->n_generic > t->n_strings) {
        set_error("lmrl_tq_create: bad argument");
        return nullptr;
    }
    // the offset tables must be monotone and stay inside what they index: the kernels walk them unchecked
    bool ok = t->str_off[0] == 0 && t->spell_off[0] == t->n_det + t->n_func + t->n_generic && t->word_off[0] == 0 &&
              t->word_off[t->n_words] == t->n_spellings && t->spell_off[t->n_spellings] == t->n_strings;
    for (int i = 0; ok && i < t->n_strings; i++) ok = t->str_off[i] <= t->str_off[i + 1];
    for (int i = 0; ok && i < t->n_spellings; i++) ok = t->spell_off[i] <= t->spell_off[i + 1];
    for (int i = 0; ok && i < t->n_words; i++) ok = t->word_off[i] <= t->word_off[i + 1] && t->prefix_len[i] >= 0 && t->prefix_len[i] <= t->prefix_cap;
    if (!ok) {
        set_error("lmrl_tq_create: inconsistent offset tables");
        return nullptr;
    }
    auto *c = new lmrl_tq_ctx();
    c->n_det = t->n_det; c->n_func = t->n_func; c->n_generic = t->n_generic; c->n_words = t->n_words; c->prefix_cap = t->prefix_cap;
    c->vocab = t->vocab; c->eos = t->eos_token; c->oracle_eos = t->oracle_eos_token;
    c->G = t->max_new_tokens; c->OG = t->oracle_max_new_tokens; c->T = t->max_turns; c->Q = t->max_new_tokens + 1;
    c->bytes_h.assign(t->bytes, t->bytes + t->str_off[t->n_strings]);
    if (c->bytes_h.empty()) c->bytes_h.push_back(0);
    c->str_off_h.assign(t->str_off, t->str_off + t->n_strings + 1);
    c->spell_off_h.assign(t->spell_off, t->spell_off + t->n_spellings + 1);
    c->word_off_h.assign(t->word_off, t->word_off + t->n_words + 1);
    c->tok_blen_h.assign(t->tok_blen, t->tok_blen + t->vocab);
    c->prefix_h.assign(t->prefix, t->prefix + (size_t)t->n_words * t->prefix_cap);
    c->prefix_len_h.assign(t->prefix_len, t->prefix_len + t->n_words);
    c->suffix_h.assign(t->suffix, t->suffix + t->suffix_len);
    c->invalid_h.assign(t->invalid_question, t->invalid_question + t->invalid_len);
    c->init_h.assign(t->initial, t->initial + t->initial_len);
    c->yes_h.assign(t->yes, t->yes + t->yes_len);
    c->no_h.assign(t->no, t->no + t->no_len);
    if (host_only) return c;
    auto up = [](auto **dst, const auto &v) {
        const size_t bytes = (v.size() ? v.size() : 1) * sizeof(v[0]);
        return hipMalloc((void **)dst, bytes) == hipSuccess && (v.empty() || hipMemcpy(*dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice) == hipSuccess);
    };
    ok = up(&c->bytes_d, c->bytes_h) && up(&c->str_off_d, c->str_off_h) && up(&c->spell_off_d, c->spell_off_h) && up(&c->word_off_d, c->word_off_h) &&
         up(&c->tok_blen_d, c->tok_blen_h) && up(&c->prefix_d, c->prefix_h) && up(&c->prefix_len_d, c->prefix_len_h) && up(&c->suffix_d, c->suffix_h) &&
         up(&c->invalid_d, c->invalid_h) && up(&c->init_d, c->init_h) && up(&c->yes_d, c->yes_h) && up(&c->no_d, c->no_h);
    if (!ok) {
        set_error("lmrl_tq_create: device allocation/copy failed (is a GPU visible?)");
        lmrl_tq_destroy(c);
        return nullptr;
    }
    c->device = true;
    return c;
}

void lmrl_tq_destroy(lmrl_tq_ctx *c) {
    if (!c) return;
    void *ptrs[] = {c->bytes_d, c->tok_blen_d, c->invalid_d, c->str_off_d, c->spell_off_d, c->word_off_d, c->prefix_d, c->prefix_len_d, c->suffix_d, c->init_d,
                    c->yes_d, c->no_d};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete c;
}

#define TQ_DEVICE(c, what) LMRL_REQUIRE((c) && (c)->device, what ": needs a context created with host_only = 0")
static bool traj_ok(const lmrl_tq_ctx *c, const lmrl_tq_traj *tr) {
    return tr && tr->hist && tr->o_prompt && tr->o_prev && tr->flags && tr->hcap >= (int)c->init_h.size() && tr->pcap > 0;
}

int lmrl_tq_reset(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, const uint64_t *seeds_d, const uint8_t *deterministic_d, const uint32_t *draws_d, int n_live,
                  int32_t *guesser_len_d, int32_t *oracle_len_d, int n, void *stream) {
    TQ_DEVICE(c, "lmrl_tq_reset");
    LMRL_REQUIRE(traj_ok(c, tr) && seeds_d && draws_d && guesser_len_d && oracle_len_d && n > 0 && n_live >= 0 && n_live <= n, "lmrl_tq_reset: bad argument");
    hipLaunchKernelGGL(tq_reset_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, as_stream(stream), *tr, dims_of(c), seeds_d, deterministic_d, draws_d, c->n_words,
                       n_live, guesser_len_d, oracle_len_d, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_tq_question(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int keep_generated, int32_t *guesser_len_d, int32_t *oracle_len_d, int n, void *stream) {
    TQ_DEVICE(c, "lmrl_tq_question");
    LMRL_REQUIRE(traj_ok(c, tr) && guesser_len_d && oracle_len_d && n > 0, "lmrl_tq_question: bad argument");
    hipLaunchKernelGGL(tq_question_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, as_stream(stream), *tr, tables_of(c, false, false), dims_of(c), keep_generated,
                       guesser_len_d, oracle_len_d, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_tq_oracle_prompt(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int j, int chunk, int n_chunks, int32_t *chunk_tok_d, int32_t *chunk_cnt_d, int n, void *stream) {
    TQ_DEVICE(c, "lmrl_tq_oracle_prompt");
    LMRL_REQUIRE(traj_ok(c, tr) && chunk_tok_d && chunk_cnt_d && n > 0 && chunk > 0 && j >= 0 && j < n_chunks, "lmrl_tq_oracle_prompt: bad argument");
    hipLaunchKernelGGL(tq_chunk_kernel, dim3(ceil_div((long)n * chunk, 256)), dim3(256), 0, as_stream(stream), tr->o_prompt, tr->pcap, tr->o_keep, tr->o_len, 1, j,
                       chunk, n_chunks * chunk, tr->flags, 1, chunk_tok_d, chunk_cnt_d, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_tq_history_chunk(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int j, int chunk, int n_chunks, int32_t *chunk_tok_d, int32_t *chunk_cnt_d, int n, void *stream) {
    TQ_DEVICE(c, "lmrl_tq_history_chunk");
    LMRL_REQUIRE(traj_ok(c, tr) && chunk_tok_d && chunk_cnt_d && n > 0 && chunk > 0 && j >= 0 && j < n_chunks, "lmrl_tq_history_chunk: bad argument");
    hipLaunchKernelGGL(tq_chunk_kernel, dim3(ceil_div((long)n * chunk, 256)), dim3(256), 0, as_stream(stream), tr->hist, tr->hcap, tr->feed_start, tr->feed_len, 0, j,
                       chunk, n_chunks * chunk, tr->flags, 8, chunk_tok_d, chunk_cnt_d, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_tq_answer(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, const int8_t *scripted_d, int script_turns, int n, void *stream) {
    TQ_DEVICE(c, "lmrl_tq_answer");
    LMRL_REQUIRE(traj_ok(c, tr) && n > 0 && (!scripted_d || script_turns > 0), "lmrl_tq_answer: bad argument");
    hipLaunchKernelGGL(tq_answer_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, as_stream(stream), *tr, tables_of(c, false, true), dims_of(c), scripted_d, script_turns, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_tq_judge(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int device_judge, int max_conversation_length, int n, void *stream) {
    TQ_DEVICE(c, "lmrl_tq_judge");
    LMRL_REQUIRE(traj_ok(c, tr) && n > 0 && max_conversation_length > 0, "lmrl_tq_judge: bad argument");
    hipLaunchKernelGGL(tq_judge_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, as_stream(stream), *tr, tables_of(c, false, false), dims_of(c), device_judge,
                       max_conversation_length, n);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

int lmrl_tq_ppo_records(lmrl_tq_ctx *c, const lmrl_tq_traj *tr, int n, int cap, int32_t *tokens_d, uint8_t *is_action_d, float *reward_d, int32_t *n_tok_d,
                        uint8_t *done_d, void *stream) {
    TQ_DEVICE(c, "lmrl_tq_ppo_records");
    LMRL_REQUIRE(traj_ok(c, tr) && n > 0 && cap > 0 && tokens_d && is_action_d && reward_d && n_tok_d && done_d, "lmrl_tq_ppo_records: bad argument");
    hipLaunchKernelGGL(tq_ppo_records_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, as_stream(stream), *tr, dims_of(c), n, cap, tokens_d, is_action_d, reward_d, n_tok_d,
                       done_d);
    LMRL_CHECK_LAUNCH();
    return LMRL_OK;
}

// ---- host faces of the text rules (no GPU needed): the same tq_core.h functions on host memory
int lmrl_tq_host_question(const lmrl_tq_ctx *c, const int32_t *ids, int n, uint8_t *question_out, int cap, int32_t *strip_range) {
    if (!c || (!ids && n > 0) || n < 0 || !question_out || cap < n + 1 || !strip_range) return -1;
    int b, e;
    const int len = lmrl_tq::question_from_ids(tables_of(c, true, false), ids, n, question_out, cap, &b, &e);
    strip_range[0] = b; strip_range[1] = e;
    return len;
}

int lmrl_tq_host_oracle_prompt(const lmrl_tq_ctx *c, int word, const uint8_t *question, int n, int32_t *out, int cap) {
    if (!c || word < 0 || word >= c->n_words || (!question && n > 0) || n < 0 || !out) return -1;
    return oracle_prompt(c->prefix_h.data() + (size_t)word * c->prefix_cap, c->prefix_len_h[word], question, n, c->suffix_h.data(), (int)c->suffix_h.size(), out, cap);
}

int lmrl_tq_host_answer(const lmrl_tq_ctx *c, const uint8_t *question, int qn, const int32_t *ids, int n) {
    if (!c || (!question && qn > 0) || qn < 0 || (!ids && n > 0) || n < 0) return -1;
    std::vector<uint8_t> text((size_t)n + 1);
    return lmrl_tq::answer_from_ids(tables_of(c, true, true), question, qn, ids, n, text.data(), n);
}

int lmrl_tq_host_is_done(const lmrl_tq_ctx *c, int word, const uint8_t *question, int n, int *judgeable) {
    if (!c || word < 0 || word >= c->n_words || (!question && n > 0) || n < 0 || !judgeable) return -1;
    return lmrl_tq::is_done(tables_of(c, true, false), word, question, n, judgeable) ? 1 : 0;
}

int lmrl_tq_host_draw_word(uint64_t seed, int deterministic, int n_words) {
    if (n_words <= 0) return -1;
    if (deterministic) return (int)(seed % (uint64_t)n_words);
    std::vector<uint32_t> state(kMtN + 1), table(kMtN);
    mt_init_table(table.data());
    MtRef r = mt_ref(state.data(), 1, 0);
    mt_seed(r, seed, table.data());
    return (int)mt_randbelow(r, (uint32_t)n_words);
}

}  // extern "C"
