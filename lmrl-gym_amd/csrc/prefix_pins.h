// prefix_pins.h — the model handle's list of pinned prompt prefixes (lmrl_gpt2_pin_prefix, csrc/gpt2.hip).  Plain C++: no HIP in here, so the
// list handling builds and runs on a CPU (tests/prefix_pins_harness.cpp) with the forward stubbed out.
//
// A pin names the caller-owned buffers of a 1-env KV session whose cache holds the K/V rows of a fixed token prefix.  Those rows are a derived
// product of the weights, like the LayerNorm-folded weight copies: lmrl_gpt2_refresh re-runs the prefill of every pin after it has re-derived
// the folded copies.  Every writer of the weights has to call refresh, so a pinned prefix cannot go stale without the folded weights going stale.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace lmrl {

constexpr int kPinChunk = 8;   // tokens per prefill forward (the chunk width of the sessions' per-turn forwards)

struct PrefixPin {
    void *kv_d; int tmax; void *ws_d;          // the session's cache and its workspace for 1 env x kPinChunk slots
    const int32_t *tokens_d; int n_tokens;     // device tokens, readable up to the next multiple of kPinChunk
    int32_t *len_d; void *last_hidden_d;       // the session's length word and last hidden state (optional)
    unsigned flags;                            // LMRL_FWD_* of the session
};

struct PrefixPinList {
    std::vector<PrefixPin> pins;

    int find(const void *kv_d) const {
        for (size_t i = 0; i < pins.size(); i++)
            if (pins[i].kv_d == kv_d) return (int)i;
        return -1;
    }
    // nullptr: added; otherwise why not
    const char *add(const PrefixPin &p) {
        if (!p.kv_d || !p.ws_d || !p.tokens_d || !p.len_d) return "null pointer";
        if (p.n_tokens <= 0 || p.tmax <= 0 || p.n_tokens > p.tmax) return "the prefix must have 1 .. tmax tokens";
        if (find(p.kv_d) >= 0) return "this cache is already pinned (unpin it first)";
        pins.push_back(p);
        return nullptr;
    }
    bool remove(const void *kv_d) {
        const int i = find(kv_d);
        if (i < 0) return false;
        pins.erase(pins.begin() + i);
        return true;
    }
    void clear() { pins.clear(); pins.shrink_to_fit(); }
};

// Prefill of one pin: len := 0, then one forward per kPinChunk tokens.  `ops` supplies zero_len(pin) and forward_chunk(pin, tokens, n), both
// returning 0 on success; the first failure stops the prefill and is returned.
template <class Ops>
int prefix_pin_prefill(const PrefixPin &p, Ops &ops) {
    if (int rc = ops.zero_len(p)) return rc;
    for (int t0 = 0; t0 < p.n_tokens; t0 += kPinChunk) {
        const int n = p.n_tokens - t0 < kPinChunk ? p.n_tokens - t0 : kPinChunk;
        if (int rc = ops.forward_chunk(p, p.tokens_d + t0, n)) return rc;
    }
    return 0;
}

template <class Ops>
int prefix_pins_refresh(const PrefixPinList &l, Ops &ops) {
    for (const PrefixPin &p : l.pins)
        if (int rc = prefix_pin_prefill(p, ops)) return rc;
    return 0;
}

}  // namespace lmrl
