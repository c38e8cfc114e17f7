// Stand-alone host program over lmrl-gym_amd/csrc/prefix_pins.h: the model handle's pin list with the forward stubbed out.
// Built and run by tests/test_prefix_pins_host.py under -fsanitize=address,undefined; exit status 0 and "ok" on success.
#include "../lmrl-gym_amd/csrc/prefix_pins.h"

#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>

using namespace lmrl;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct Call { const void *kv; long tok_off; int n; };   // n < 0: zero_len

struct StubOps {
    std::vector<Call> calls;
    const void *fail_on = nullptr;   // forward_chunk of this cache fails with 7
    int zero_len(const PrefixPin &p) {
        *p.len_d = 0;
        calls.push_back({p.kv_d, 0, -1});
        return 0;
    }
    int forward_chunk(const PrefixPin &p, const int32_t *tokens, int n) {
        if (p.kv_d == fail_on) return 7;
        calls.push_back({p.kv_d, (long)(tokens - p.tokens_d), n});
        *p.len_d += n;
        return 0;
    }
};

int main() {
    char kv_a[4], kv_b[4], ws[4], hid[4];
    int32_t tok[16] = {0}, len_a = 99, len_b = 99;
    const PrefixPin a{kv_a, 16, ws, tok, 11, &len_a, hid, 0u}, b{kv_b, 16, ws, tok, 8, &len_b, nullptr, 4u};

    // a null pin, an empty and an overlong prefix are refused and leave the list as it was
    {
        PrefixPinList l;
        PrefixPin p = a; p.kv_d = nullptr; CHECK(l.add(p) != nullptr);
        p = a; p.ws_d = nullptr; CHECK(l.add(p) != nullptr);
        p = a; p.tokens_d = nullptr; CHECK(l.add(p) != nullptr);
        p = a; p.len_d = nullptr; CHECK(l.add(p) != nullptr);
        p = a; p.n_tokens = 0; CHECK(l.add(p) != nullptr);
        p = a; p.n_tokens = 17; CHECK(l.add(p) != nullptr);
        p = a; p.last_hidden_d = nullptr; CHECK(l.add(p) == nullptr);      // the hidden state is optional
        CHECK(l.pins.size() == 1);
    }
    PrefixPinList l;
    CHECK(l.add(a) == nullptr && l.add(b) == nullptr && l.pins.size() == 2);
    const char *why = l.add(a);                                             // the same cache twice
    CHECK(why && strstr(why, "already pinned") && l.pins.size() == 2);
    CHECK(l.find(kv_a) == 0 && l.find(kv_b) == 1 && l.find(ws) == -1);

    // prefill: len := 0, then chunks of 8 tokens, the last one short
    StubOps ops;
    CHECK(prefix_pin_prefill(a, ops) == 0 && len_a == 11);
    CHECK(ops.calls.size() == 3 && ops.calls[0].n == -1 && ops.calls[1].tok_off == 0 && ops.calls[1].n == 8 && ops.calls[2].tok_off == 8 &&
          ops.calls[2].n == 3);

    // refresh: every pin, in pin order
    ops.calls.clear(); len_a = len_b = 99;
    CHECK(prefix_pins_refresh(l, ops) == 0 && len_a == 11 && len_b == 8);
    CHECK(ops.calls.size() == 5 && ops.calls[0].kv == kv_a && ops.calls[3].kv == kv_b && ops.calls[4].n == 8);

    // a failing forward stops the refresh and comes back as it is
    ops.calls.clear(); ops.fail_on = kv_a; len_b = 99;
    CHECK(prefix_pins_refresh(l, ops) == 7 && len_b == 99);
    ops.fail_on = nullptr;

    // unpin: refresh no longer touches that pin; unknown caches are reported
    CHECK(l.remove(kv_a) && !l.remove(kv_a) && !l.remove(nullptr) && l.pins.size() == 1);
    ops.calls.clear(); len_a = 99; len_b = 99;
    CHECK(prefix_pins_refresh(l, ops) == 0 && len_a == 99 && len_b == 8);
    for (const Call &c : ops.calls) CHECK(c.kv == kv_b);
    CHECK(l.add(a) == nullptr);                                             // and the cache can be pinned again

    // destroy with pins alive: the handle clears the list, then goes away
    {
        auto owner = std::make_unique<PrefixPinList>();
        CHECK(owner->add(a) == nullptr && owner->add(b) == nullptr);
        owner->clear();
        CHECK(owner->pins.empty() && owner->find(kv_a) == -1);
        ops.calls.clear();
        CHECK(prefix_pins_refresh(*owner, ops) == 0 && ops.calls.empty());
        CHECK(owner->add(b) == nullptr);                                    // deleted with a pin in it
    }
    l.clear();
    CHECK(l.pins.empty());
    puts("ok");
    return 0;
}
