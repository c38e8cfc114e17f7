"""GPU tier: the pinned header prefix and the one-launch reduce + accept + embed tail of the Wordle rollout.

Both are pure launch removals: every check here is `torch.equal` against the path they replace (the in-episode header prefill; the three
launches sample_reduce / tok_accept / embed_stats).  Model: 2 layers, d_model 128 (LN-folded path), vocabulary 9000 (71 LM-head tiles: lanes of
the partial merge with one and with two partials); batches 130 (a partial 4-row block, a partial 128-row LM-head tile) and 5."""
import ctypes

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VOCAB, G = 9000, 7          # max_new_tokens 7: a steered action ends on its '\n' at k = 5, so k = 6 runs with every row inactive
TRAJ = ("tokens", "is_action", "reward", "n_tok", "gen", "gen_len", "gen_active", "env_done", "pend_newline", "n_steps", "ep_reward")


def _table():
    from lmrl_gym_amd.rollout import WordleTokenTable
    lf, ls = list(range(26)), list(range(26, 52))
    t = WordleTokenTable(newline=55, pad=VOCAB, letter_first=lf, letter_sp=ls, sym_first=[lf[6], lf[24], lf[1]], sym_sp=[ls[6], ls[24], ls[1]],
                         header=[52, 53, 54, 55])
    t.strings = {52: "Word", 53: "le", 54: ":", 55: "\n"}
    for i in range(26):
        t.strings[i] = chr(97 + i)
        t.strings[26 + i] = " " + chr(97 + i)
    return t


def _weights(cfg, seed):
    from lmrl_gym_amd.gpt2 import init_hf_style_state_dict
    """Random weights whose samples DEPEND on them: logits of standard deviation ~1.8 beside the Gumbel noise's 1.3 (wte x 8), and positions that
    outweigh the token in the residual stream (wpe x 40) — with the tied embedding alone the input token's own logit (~20) would win every draw,
    i.e. every action would be the '\n' that ends the header, whatever the weights."""
    sd = init_hf_style_state_dict(cfg, seed=seed)
    sd["wte.weight"] = sd["wte.weight"] * 8
    sd["wpe.weight"] = sd["wpe.weight"] * 40
    return sd


@pytest.fixture(scope="module")
def setup():
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.envs import wordle as W
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine
    dev = _lib.require_gpu()
    cfg = GPT2Config(2, 2, 128, 512, VOCAB, 128)
    sd1, sd2 = _weights(cfg, 5), _weights(cfg, 6)
    return dev, cfg, sd1, sd2, GPT2Engine(cfg, sd1, dev), W.Vocabulary.builtin("wordle_official_400.txt"), _table()


def _guesses(vocab, B, dev, seed=1):
    from lmrl_gym_amd.envs import wordle as W
    rng = np.random.RandomState(seed)
    words = vocab.all_vocab
    packed = np.array([[W.pack_guess(words[i]) for i in rng.randint(0, len(words), size=B)] for _ in range(6)], dtype=np.uint32)
    return torch.from_numpy(packed.view(np.int32)).to(dev)


def _header_kv(ro):
    e = ro.eng.cfg
    return ro.ses.kv.view(torch.int16).view(e.n_layer, 2, ro.B, ro.ses.tmax, e.d_model)[:, :, :, : len(ro.tokens.header)].clone()


def _result(ro, valid_only=False):
    """The episode's outputs.  `valid_only`: for engines whose EARLIER episodes differed — the record arrays are compared up to each env's n_tok
    (slots past it keep what a longer earlier episode left there) and `gen`, whose rows past the last action's length are such leftovers, not at all."""
    torch.cuda.synchronize()
    r = {**{n: ro.traj[n].clone() for n in TRAJ}, "token": ro.ses.token.clone(), "header_kv": _header_kv(ro), "len": ro.ses.len.clone()}
    if valid_only:
        del r["gen"]
        past = torch.arange(ro.cap, device=ro.dev)[None, :] >= r["n_tok"][:, None]
        for n in ("tokens", "is_action", "reward"):
            r[n][past] = 0
    return r


def _same(a, b, what):
    for n in a:
        assert torch.equal(a[n], b[n]), (what, n)


# ------------------------------------------------------------------------------------------ 1. one step: fused launch == three launches
@pytest.mark.parametrize("B", [130, 5])
@pytest.mark.parametrize("k,want_lp,temperature", [(0, False, 1.0), (0, True, 1.0), (G - 1, False, 1.0), (G - 1, True, 0.0)])
def test_fused_launch_equals_three_launches(setup, B, k, want_lp, temperature):
    """sample -> accept -> forward on a 0-LAYER model over the same embedding tables: its single-token forward is the embedding launch plus the
    final LayerNorm, so the workspace afterwards holds exactly what embed_stats_kernel wrote (x, xb, every stats slot) — compared, whole
    buffer, with the workspace the fused launch filled before a forward that was told to skip its embedding.  Some rows are steered to '\\n'
    (they end), some start with gen_active = 0."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine, SampleParams
    from lmrl_gym_amd.rollout import WordleRolloutEngine
    dev, cfg, sd1, _, _, vocab, tab = setup
    cfg0 = GPT2Config(0, 2, 128, 512, VOCAB, 128)
    eng0 = GPT2Engine(cfg0, sd1, dev)
    L = _lib.lib()
    g = torch.Generator().manual_seed(100 + B)
    hidden = torch.randn(B, cfg0.d_model, generator=g).to(torch.bfloat16).to(dev)
    lens = torch.randint(4, 40, (B,), generator=g).numpy()
    rows = torch.arange(B)
    active0 = (rows % 4 != 3).to(torch.uint8).to(dev)                                   # every fourth row starts inactive
    steer = torch.where(rows % 3 == 0, tab.newline, -1).to(torch.int32).to(dev)         # every third row is steered to '\n'
    out = []
    for fused in (False, True):
        ro = WordleRolloutEngine(eng0, vocab, B, tokens=tab, max_new_tokens=G, share_header=False)
        ses, tr, sp = ro.ses, ctypes.byref(ro._ctraj), _lib.stream_ptr()
        ses.kv = torch.zeros(256, dtype=torch.uint8, device=dev)          # a 0-layer cache has no bytes; the ABI wants an address
        ses.set_len(lens)
        ses.last_hidden.copy_(hidden)
        ses.ws[1].fill_(0x5A)                                              # so that "the other slots zero" is something the launch has to do
        ro.traj["gen_active"].copy_(active0)
        ro.traj["gen_len"].fill_(k)
        more = k < G - 1
        p = SampleParams(temperature, 0, 31, 3, 200.0, 0.0, tab.pad, None, 0.0)
        ses.sample(p, steer_tok=steer, active=ro.traj["gen_active"], want_logprob=want_lp, keep_partials=fused)
        if fused:
            _lib.check(L.lmrl_wordle_sample_accept_embed(ro._tok, tr, _lib.ptr(ses.sample_ws), cfg0.vocab_padded, tab.pad, _lib.ptr(ro.traj["gen_active"]),
                                                         _lib.ptr(ses.token), _lib.ptr(ses.logprob) if want_lp else None, k, _lib.ptr(ro.next_tok),
                                                         _lib.ptr(ro.next_cnt), _lib.ptr(ro.active), eng0._h if more else None,
                                                         _lib.ptr(ses.ws[1]) if more else None, _lib.ptr(ses.len) if more else None, B, sp), "fused")
            if more:      # x = wte[tok] + wpe[pos] is one exact fp32 add, xb its bf16 rounding: the fused launch's rows against plain indexing
                torch.cuda.synchronize()
                cnt = ro.next_cnt.bool()
                tok = torch.where(cnt, ro.next_tok, 0).long()
                pos = torch.where(cnt, ses.len, 0).long()
                x_exp = eng0.wte[tok].float() + eng0.wpe[pos].float()
                nx = B * cfg0.d_model * 4
                x = ses.ws[1][:nx].view(torch.float32).view(B, -1)
                xb = ses.ws[1][(nx + 255) // 256 * 256:][: nx // 2].view(torch.bfloat16).view(B, -1)
                assert torch.equal(x, x_exp) and torch.equal(xb, x_exp.to(torch.bfloat16))
        else:
            _lib.check(L.lmrl_wordle_tok_accept(ro._tok, tr, _lib.ptr(ses.token), k, _lib.ptr(ro.next_tok), _lib.ptr(ro.next_cnt), _lib.ptr(ro.active), B, sp),
                       "tok_accept")
        if more:
            ses.forward(ro.next_tok, ro.next_cnt, 1, pre_embedded=fused)
        torch.cuda.synchronize()
        r = {n: ro.traj[n].clone() for n in ("gen", "gen_len", "gen_active")}
        r.update(token=ses.token.clone(), next_tok=ro.next_tok.clone(), next_cnt=ro.next_cnt.clone(), active=ro.active.clone(), ws=ses.ws[1].clone(),
                 last_hidden=ses.last_hidden.clone(), len=ses.len.clone())
        if want_lp:
            r["logprob"] = ses.logprob.clone()
        out.append(r)
        ro.close()
    _same(out[0], out[1], (B, k))
    a = out[0]
    ended = active0.bool() & ~a["gen_active"].bool()
    if more:      # the case has what it is meant to have: rows that go on, rows that end on the steered '\n', rows that were never active
        assert int(a["next_cnt"].sum()) > 0 and bool(ended.any()) and bool((a["token"][ended] == tab.newline).all())
    else:
        assert int(a["next_cnt"].sum()) == 0 and torch.equal(ended, active0.bool())
    assert bool((a["token"][~active0.bool()] == tab.pad).all()) and bool((~active0.bool()).any())


# ------------------------------------------------------------------------------------------ 2. whole episodes, the four combinations
@pytest.mark.parametrize("B", [130, 5])
def test_episodes_equal_across_switches(setup, B):
    """fused on / off x pinned on / off, eager and captured, steered and unsteered: records, last tokens, header K/V rows and cache lengths."""
    from lmrl_gym_amd.rollout import WordleRolloutEngine
    dev, cfg, _, _, eng, vocab, tab = setup
    seeds = np.arange(B, dtype=np.uint64) + 40
    seeds_d = torch.from_numpy(seeds.view(np.int64)).to(dev)
    guesses = _guesses(vocab, B, dev)
    ref = {}
    for fused, pinned in ((False, False), (True, False), (False, True), (True, True)):
        for mode in ("eager", "graph"):
            for steered in (False, True):
                ro = WordleRolloutEngine(eng, vocab, B, tokens=tab, max_new_tokens=G, pin_header=pinned, fused_tail=fused)
                assert ro._fused_tail_ok(0, 0.0, False) == fused and ro.pin_header == pinned
                strength = 200.0 if steered else 0.0
                if mode == "eager":
                    ro.run_episode(seeds, temperature=1.0, sample_seed=11, scripted_guesses=guesses if steered else None, steer_strength=strength)
                else:
                    ro.capture_episode(temperature=1.0, sample_seed=11, steer_strength=strength, scripted=steered)
                    ro.replay_episode(seeds_d, guesses if steered else None)
                r = _result(ro)
                ro.close()
                if (mode, steered) not in ref:
                    ref[(mode, steered)] = r          # (fused off, pinned off): the parent's launches
                    # steered draws spell vocabulary words (actions end on '\n' at k = 5, k = 6 runs with every row inactive); a random model
                    # on its own never spells one (six bad-word rewards, every action runs to max_new_tokens)
                    assert bool((r["ep_reward"] > -60.0).all()) if steered else bool((r["ep_reward"] == -60.0).all())
                    if not steered:      # header + 6 x (max_new_tokens + forced '\n' + the observation's '\n')
                        assert int(r["n_tok"].max()) == len(tab.header) + 6 * (G + 2)
                else:
                    _same(ref[(mode, steered)], r, (fused, pinned, mode, steered))


# ------------------------------------------------------------------------------------------ 3. a captured graph after a weight push
def test_captured_episode_follows_load_params(setup):
    """The captured episode no longer prefills the header: after `load_params` its replay must still see the NEW weights' header rows."""
    from lmrl_gym_amd.gpt2 import GPT2Engine
    from lmrl_gym_amd.rollout import WordleRolloutEngine
    dev, cfg, sd1, sd2, _, vocab, tab = setup
    B = 130
    seeds_d = torch.from_numpy((np.arange(B, dtype=np.uint64) + 9).view(np.int64)).to(dev)

    def replay(ro):
        ro.g_epoch.fill_(7)           # the same noise epoch for every replay compared here
        ro.replay_episode(seeds_d)
        return _result(ro, valid_only=True)
    eng = GPT2Engine(cfg, sd1, dev)
    ro = WordleRolloutEngine(eng, vocab, B, tokens=tab, max_new_tokens=G)
    assert ro.pin_header
    ro.capture_episode(temperature=1.0, sample_seed=23)
    first = replay(ro)
    ro.load_params({k: v.to(dev) for k, v in sd2.items()})
    second = replay(ro)
    fresh = WordleRolloutEngine(GPT2Engine(cfg, sd2, dev), vocab, B, tokens=tab, max_new_tokens=G, pin_header=False)
    fresh.capture_episode(temperature=1.0, sample_seed=23)
    _same(replay(fresh), second, "second weight set")
    assert not torch.equal(first["header_kv"], second["header_kv"]) and not torch.equal(first["tokens"], second["tokens"])
    ro.load_params({k: v.to(dev) for k, v in sd1.items()})
    _same(first, replay(ro), "back to the first weight set")
    fresh.close()
    ro.close()


# ------------------------------------------------------------------------------------------ 4. pin lifecycle
def test_pin_lifecycle(setup):
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gpt2 import GPT2Engine
    dev, cfg, sd1, _, _, _, _ = setup
    eng = GPT2Engine(cfg, sd1, dev)
    L = _lib.lib()
    toks = [52, 53, 54, 55, 3, 30, 31, 32, 33, 55, 7]          # 11 tokens: two chunks
    pinned = eng.session(1, 16)
    assert pinned.pin_as_prefix(toks) == 11
    # == two KVSession.forward calls
    plain = eng.session(1, 16)
    plain.reset()
    t = torch.tensor(toks + [0] * 5, dtype=torch.int32, device=dev)
    plain.forward(t[:8], torch.tensor([8], dtype=torch.int32, device=dev), 8)
    plain.forward(t[8:], torch.tensor([3], dtype=torch.int32, device=dev), 8)
    torch.cuda.synchronize()
    assert torch.equal(pinned.kv, plain.kv) and torch.equal(pinned.len, plain.len) and torch.equal(pinned.last_hidden, plain.last_hidden)
    assert int(pinned.len[0]) == 11
    # the same cache twice is refused, with a text
    with pytest.raises(_lib.LmrlError, match="already pinned"):
        _lib.check(L.lmrl_gpt2_pin_prefix(eng._h, _lib.ptr(pinned.kv), 16, _lib.ptr(pinned.ws[8]), _lib.ptr(pinned._pin_tokens), 11, _lib.ptr(pinned.len),
                                          None, 0, _lib.stream_ptr()), "pin")
    assert b"already pinned" in L.lmrl_last_error()
    # the session itself refuses what would pull the pinned buffers from under the engine: a second pin (its token tensor stays), reset, forward
    held = pinned._pin_tokens
    with pytest.raises(_lib.LmrlError, match="already pinned"):
        pinned.pin_as_prefix(toks[:4])
    assert pinned._pin_tokens is held and pinned._pinned == 11
    with pytest.raises(_lib.LmrlError, match="pinned prefix"):
        pinned.reset()
    with pytest.raises(_lib.LmrlError, match="pinned prefix"):
        pinned.forward(t[:8], torch.tensor([8], dtype=torch.int32, device=dev), 8)
    # refresh prefills a pin again ...
    pinned.kv.zero_(); pinned.len.fill_(13)
    _lib.check(L.lmrl_gpt2_refresh(eng._h, _lib.stream_ptr()), "refresh")
    torch.cuda.synchronize()
    assert int(pinned.len[0]) == 11 and torch.equal(pinned.kv, plain.kv)
    # ... and leaves an unpinned session alone
    pinned.unpin_prefix()
    pinned.len.fill_(13)
    _lib.check(L.lmrl_gpt2_refresh(eng._h, _lib.stream_ptr()), "refresh")
    torch.cuda.synchronize()
    assert int(pinned.len[0]) == 13
    with pytest.raises(_lib.LmrlError, match="not pinned"):
        _lib.check(L.lmrl_gpt2_unpin_prefix(eng._h, _lib.ptr(pinned.kv)), "unpin")
    # a prefix longer than the cache is refused; the cache can be pinned again afterwards
    with pytest.raises(_lib.LmrlError, match="tmax"):
        pinned.pin_as_prefix(list(range(17)))
    assert pinned._pin_tokens is held and pinned._pinned == 0          # a refused pin leaves the session as it was
    assert pinned.pin_as_prefix(toks[:4]) == 4


def test_switches_are_refused_where_they_do_not_apply(setup):
    """No quiet change of path: the partials stay only where the plain reduce would have read them, and a forward skips its embedding only
    where the fused launch can have written it."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gpt2 import FWD_LN_STANDALONE, SampleParams
    dev, cfg, _, _, eng, _, tab = setup
    ses = eng.session(5, 16)
    ses.reset()
    logits = torch.empty(5, cfg.vocab_padded, dtype=torch.float32, device=dev)
    p = SampleParams(1.0, 8, 1, 0, 0.0, 0.0, tab.pad, None, 0.0)
    with pytest.raises(_lib.LmrlError, match="KEEP_PARTIALS"):
        ses.sample(p, logits_out=logits, keep_partials=True)
    assert p.flags == 0                                                # the switch travels on a copy of the caller's struct
    ses.sample(p, logits_out=logits)                                   # ... so the same struct samples normally afterwards
    from lmrl_gym_amd.gpt2 import FWD_RAGGED_ALWAYS, FWD_SKINNY
    takes = lambda b, f: _lib.lib().lmrl_gpt2_forward_takes_pre_embedded(eng._h, b, f)
    assert takes(130, 0) == 1 and takes(2048, 0) == 0 and takes(130, FWD_LN_STANDALONE) == 0 and takes(130, FWD_RAGGED_ALWAYS) == 0 and takes(5, FWD_SKINNY) == 0
    tok, cnt = torch.zeros(5 * 8, dtype=torch.int32, device=dev), torch.ones(5, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.LmrlError, match="pre_embedded"):
        ses.forward(tok, cnt, 8, pre_embedded=True)
    standalone = eng.session(5, 16, FWD_LN_STANDALONE)
    standalone.reset()
    with pytest.raises(_lib.LmrlError, match="PRE_EMBEDDED"):
        standalone.forward(tok[:5], cnt, 1, pre_embedded=True)
    torch.cuda.synchronize()
