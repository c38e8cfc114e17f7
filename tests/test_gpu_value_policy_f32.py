"""GPU tier: the ILQL and MC-returns value policies on the fp32 rollout engine (`GPT2EngineF32`, "f32" and "bf16x3" modes).

The reference evaluates its value policies in float32 by default (wordle/ilql/eval_ilql_gpt2.py:36, wordle/mc/eval_mc_gpt2.py:103-116):
logits = pi_beta + beta * min(Q1, Q2), or pi_beta + beta * Q for the MC policy (value_rl_base/gpt2/generation.py:100-119).  Covered here:
  * `lmrl_value_head_logits_f32` (csrc/value_head_f32.hip) against a float64 restatement within a k-ordered fp32 bound, and bit for bit against
    `lmrl_sgemm` of the same operands (beta = 0: pi_beta alone; a zero pi_beta operand and beta = 1: the min of the two Q products);
  * every sampled token of a steered GPT-2-small Wordle rollout against the float64 oracle (two transformers, two MLP heads) and the reference's
    jax random stream, in both matmul modes and both policy forms, with the Q heads shown to change the draws;
  * hipGraph replay, the dual-stream forwards and `text_env_eval(concurrent=2)` lanes, bit for bit against their plain counterparts;
  * the text-protocol policies (`GPT2ValuePolicy`, `GPT2PPOPolicy`) on fp32 engines with prefix reuse (`KVSessionF32.set_len`);
  * top-k / top-p on the value head against `oracle.warpers`; refusals of mixed engines and head layouts; the harness's --policy-engine."""
import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    from lmrl_gym_amd import _lib
    return _lib.require_gpu()


def _mlp_params(d, V, seed, w2_scale=None, b2_scale=0.1):
    """MLPHead params with Q values of unit-ish spread on LayerNorm-scale inputs (so that beta * Q moves the draws)."""
    g = torch.Generator().manual_seed(seed)
    return {"dense1.kernel": torch.randn(d, d, generator=g) / d ** 0.5, "dense1.bias": torch.randn(d, generator=g) * 0.1,
            "dense2.kernel": torch.randn(d, V, generator=g) * (w2_scale if w2_scale is not None else 1.0 / d ** 0.5),
            "dense2.bias": torch.randn(V, generator=g) * b2_scale}


def _head_call(L, h, wte, q1, q2, beta, m, d, Vp, out):
    from lmrl_gym_amd import _lib
    p = _lib.ptr
    return L.lmrl_value_head_logits_f32(p(h), p(wte), p(q1[0]), p(q1[1]), p(q1[2]), p(q2[0]) if q2 else None, p(q2[1]) if q2 else None,
                                        p(q2[2]) if q2 else None, float(beta), m, d, Vp, p(out), Vp, _lib.stream_ptr())


@pytest.mark.parametrize("m,d,Vp", [(1, 768, 50304), (37, 768, 50304), (1024, 768, 50304), (37, 128, 1280), (1024, 128, 1280)])
def test_value_head_kernel_vs_float64_and_sgemm(dev, m, d, Vp):
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.train import ops
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(m * 7 + d)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g, device=dev) * sc
    V = Vp - 47                                         # a padded vocabulary: zero weight rows and biases past V
    pad = lambda w: torch.cat([w[:V], torch.zeros(Vp - V, *w.shape[1:], device=dev)]).contiguous()
    h, qh1, qh2 = r(m, d), r(m, d).relu(), r(m, d).relu()
    wte, w2a, w2b = pad(r(Vp, d, sc=0.05)), pad(r(Vp, d, sc=d ** -0.5)), pad(r(Vp, d, sc=d ** -0.5))
    b2a, b2b = pad(r(Vp, sc=0.3)), pad(r(Vp, sc=0.3))
    beta = 2.5
    out, out2 = (torch.full((m, Vp), float("nan"), device=dev) for _ in range(2))
    D = lambda x: x.double()
    pi = D(h) @ D(wte).t()
    api = D(h).abs() @ D(wte).abs().t()
    for form in ("ilql", "mc"):
        q2 = (qh2, w2b, b2b) if form == "ilql" else None
        _lib.check(_head_call(L, h, wte, (qh1, w2a, b2a), q2, beta, m, d, Vp, out), "lmrl_value_head_logits_f32")
        _lib.check(_head_call(L, h, wte, (qh1, w2a, b2a), q2, beta, m, d, Vp, out2), "lmrl_value_head_logits_f32")
        torch.cuda.synchronize()
        assert torch.equal(out, out2), form                                   # deterministic
        q1r, aq1 = D(qh1) @ D(w2a).t() + D(b2a), D(qh1).abs() @ D(w2a).abs().t() + D(b2a).abs()
        if q2 is None:
            q, aq = q1r, aq1
        else:
            q2r, aq2 = D(qh2) @ D(w2b).t() + D(b2b), D(qh2).abs() @ D(w2b).abs().t() + D(b2b).abs()
            q, aq = torch.minimum(q1r, q2r), torch.maximum(aq1, aq2)
        ref = pi + beta * q
        bound = 8 * U * (api + beta * aq) + U * ref.abs() + 1e-30
        ratio = float(((D(out) - ref).abs() / bound).max())
        print(f"m={m} d={d} {form}: max |err| / (8 u sum|ab| + u |ref|) = {ratio:.3f}")
        assert ratio <= 1.0, (form, ratio)
        # beta = 0: pi_beta alone, bit-equal to lmrl_sgemm of the same operands
        ref_pi = torch.empty(m, Vp, device=dev)
        ops.sgemm(h, wte, ref_pi, m, Vp, d, trans_b=True, lda=d, ldb=d, ldc=Vp)
        _lib.check(_head_call(L, h, wte, (qh1, w2a, b2a), q2, 0.0, m, d, Vp, out), "lmrl_value_head_logits_f32")
        assert torch.equal(out, ref_pi), form
        # a zero pi_beta operand and beta = 1: the Q products (+ bias) and their min, bit-equal to lmrl_sgemm
        zs = torch.zeros(m, Vp, device=dev), torch.zeros(m, Vp, device=dev)
        ops.sgemm(qh1, w2a, zs[0], m, Vp, d, trans_b=True, lda=d, ldb=d, ldc=Vp, bias=b2a)
        ops.sgemm(qh2, w2b, zs[1], m, Vp, d, trans_b=True, lda=d, ldb=d, ldc=Vp, bias=b2b)
        _lib.check(_head_call(L, torch.zeros_like(h), wte, (qh1, w2a, b2a), q2, 1.0, m, d, Vp, out), "lmrl_value_head_logits_f32")
        assert torch.equal(out, zs[0] if q2 is None else torch.minimum(zs[0], zs[1])), form


def test_value_head_kernel_refuses_bad_shapes(dev):
    from lmrl_gym_amd import _lib
    L = _lib.lib()
    t = lambda *s: torch.zeros(*s, device=dev)
    h, w, b, out = t(4, 128), t(1280, 128), t(1280), t(4, 1280)
    q = (h, w, b)
    assert _head_call(L, h, w, q, q, 1.0, 4, 128, 1280, out) == 0
    for m, d, Vp in ((0, 128, 1280), (4, 100, 1280), (4, 128, 1200)):
        assert _head_call(L, h, w, q, q, 1.0, m, d, Vp, out) != 0
        assert b"lmrl_value_head_logits_f32" in L.lmrl_last_error()
    p = _lib.ptr
    rc = L.lmrl_value_head_logits_f32(p(h), p(w), p(h), p(w), p(b), p(h), None, p(b), 1.0, 4, 128, 1280, p(out), 1280, _lib.stream_ptr())
    assert rc != 0 and b"all given" in L.lmrl_last_error()
    rc = L.lmrl_value_head_logits_f32(p(h), p(w), p(h), p(w), p(b), None, None, None, 1.0, 4, 128, 1280, p(out), 1000, _lib.stream_ptr())
    assert rc != 0


def _gpt2_small_value_policy(dev, matmul, form):
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    from lmrl_gym_amd.policies import heads_to_engine_layout
    cfg = GPT2Config.gpt2_small()
    sd, sd_v = init_hf_style_state_dict(cfg, seed=0), init_hf_style_state_dict(cfg, seed=1)
    pi, vb = GPT2EngineF32(cfg, sd, dev, matmul=matmul), GPT2EngineF32(cfg, sd_v, dev, matmul=matmul)
    h1, h2 = _mlp_params(cfg.d_model, cfg.vocab, 11), (_mlp_params(cfg.d_model, cfg.vocab, 12) if form == "ilql" else None)
    lay = lambda hp: None if hp is None else heads_to_engine_layout(hp, cfg.vocab_padded, dev, engine=pi)
    return cfg, sd, sd_v, pi, vb, h1, h2, lay(h1), lay(h2)


@pytest.mark.parametrize("form", ["ilql", "mc"])
@pytest.mark.parametrize("matmul,tie", [("f32", 2e-4), ("bf16x3", 3e-3)])
def test_value_rollout_every_sampled_token_equals_float64_oracle_with_jax_stream(dev, matmul, tie, form):
    from lmrl_gym_amd.envs import wordle as W
    from lmrl_gym_amd.rollout import WordleRolloutEngine
    from oracle import gpt2 as O, jax_random as JR, rl
    cfg, sd, sd_v, pi, vb, h1, h2, l1, l2 = _gpt2_small_value_policy(dev, matmul, form)
    vocab = W.Vocabulary.builtin("wordle_official_400.txt")
    words = vocab.all_vocab
    B, STEER, SEED, BETA = 64, 12.5, 2024, 3.0
    ro = WordleRolloutEngine(pi, vocab, B, max_new_tokens=6, bad_word_reward=-10.0, value_engine=vb, q1_head=l1, q2_head=l2, beta=BETA)
    tab = ro.tokens
    rng = np.random.RandomState(5)
    packed = np.array([W.pack_guess(w) for w in words], dtype=np.uint32)
    g_np = packed[rng.randint(0, len(packed), size=(6, B))]
    guesses = torch.from_numpy(g_np.view(np.int32)).to(dev)
    seeds = np.arange(B, dtype=np.uint64) + 7
    ro.run_episode(seeds, temperature=1.0, sample_seed=SEED, scripted_guesses=guesses, steer_strength=STEER, sampler="jax")
    torch.cuda.synchronize()
    trajs = ro.token_trajectories()
    ro.close()
    # the action runs of every env (token positions, turn); the env outcomes themselves are pinned by tests/test_gpu_f32_engine.py
    runs_of = []
    for b in range(B):
        ia = trajs[b][1]
        runs, pos, turn = [], len(tab.header), 0
        while pos < len(ia):
            start = pos
            while pos < len(ia) and ia[pos]:
                pos += 1
            runs.append((start, pos, turn))
            turn += 1
            while pos < len(ia) and not ia[pos]:
                pos += 1
        runs_of.append(runs)
    V = cfg.vocab
    maxlen = max(len(t[0]) for t in trajs)
    ids = torch.zeros(B, maxlen, dtype=torch.int64)
    for b in range(B):
        ids[b, : len(trajs[b][0])] = torch.from_numpy(trajs[b][0].astype(np.int64))
    logits = O.forward(sd, ids, cfg.n_head)[:, :, :V]                       # float64, right padding + causal mask: prefixes unaffected
    _, hid = O.forward(sd_v, ids, cfg.n_head, return_hidden=True)
    hd = hid.to(dev)
    qs = [None if hp is None else rl.mlp_head(hd, *(hp[k].to(dev) for k in ("dense1.kernel", "dense1.bias", "dense2.kernel", "dense2.bias")))
          for hp in (h1, h2)]
    pert = rl.value_rl_logits(logits.to(dev), qs[0], qs[1], BETA).cpu().numpy()
    logits = logits.numpy()
    pol_key = JR.prng_key(SEED)
    checked = near_tie = moved = 0
    for turn in range(6):
        pol_key, new_key = JR.split(pol_key)
        keys = JR.hf_flax_sample_keys(new_key, 6)
        for k in range(6):
            noise = JR.gumbel(keys[k], (B, V)).astype(np.float64)
            for b in range(B):
                run = next((r for r in runs_of[b] if r[2] == turn), None)
                if run is None or k >= min(run[1] - run[0], 6):
                    continue
                start = run[0]
                c = (int(g_np[turn, b]) >> (5 * k)) & 31
                st = tab.newline if k >= 5 else (tab.letter_first[c % 26] if k == 0 else tab.letter_sp[c % 26])
                score = pert[b, start + k - 1] + noise[b]
                score[st] += STEER
                top2 = np.partition(score, -2)[-2:]
                if top2[1] - top2[0] < tie:
                    near_tie += 1
                    continue
                checked += 1
                assert int(score.argmax()) == int(trajs[b][0][start + k]), (turn, k, b)
                z_pi = logits[b, start + k - 1] + noise[b]
                z_pi[st] += STEER
                moved += int(z_pi.argmax()) != int(score.argmax())
    print(f"{matmul} {form}: {checked} draws checked, {near_tie} near ties, Q heads moved the argmax in {moved}")
    assert checked >= 1200 and near_tie <= (0.005 if matmul == "f32" else 0.03) * (checked + near_tie), (checked, near_tie)
    assert moved >= 0.2 * checked, (moved, checked)


def _small_value_rollout(dev, B, matmul="f32", **kw):
    from lmrl_gym_amd.envs import wordle as W
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    from lmrl_gym_amd.policies import heads_to_engine_layout
    from lmrl_gym_amd.rollout import WordleRolloutEngine
    cfg = GPT2Config(2, 12, 768, 3072, 50257, 128)           # d = 768: the Q heads' dense1 takes lmrl_sgemm's split-K path at B = 256
    pi = GPT2EngineF32(cfg, init_hf_style_state_dict(cfg, seed=3), dev, matmul=matmul)
    vb = GPT2EngineF32(cfg, init_hf_style_state_dict(cfg, seed=4), dev, matmul=matmul)
    assert pi.q_hidden_ws(B) is not None
    lay = lambda s: heads_to_engine_layout(_mlp_params(cfg.d_model, cfg.vocab, s), cfg.vocab_padded, dev, engine=pi)
    vocab = W.Vocabulary.builtin("wordle_official_400.txt")
    ro = WordleRolloutEngine(pi, vocab, B, max_new_tokens=6, bad_word_reward=-10.0, value_engine=vb, q1_head=lay(21), q2_head=lay(22), beta=3.0, **kw)
    return ro, vocab


def test_f32_value_policy_graph_streams_and_lanes_are_bit_identical(dev):
    from lmrl_gym_amd.envs import wordle as W
    B = 256
    ro, vocab = _small_value_rollout(dev, B)
    rng = np.random.RandomState(3)
    packed = np.array([W.pack_guess(w) for w in vocab.all_vocab], dtype=np.uint32)
    guesses = torch.from_numpy(packed[rng.randint(0, len(packed), size=(6, B))].view(np.int32)).to(dev)
    seeds = (torch.arange(B, dtype=torch.int64) + 900).to(dev)
    kw = dict(temperature=1.0, sample_seed=11, steer_strength=12.5)
    keys = ("tokens", "is_action", "reward", "n_tok", "n_steps", "ep_reward", "env_done")
    snap = lambda: {k: ro.traj[k].clone() for k in keys}
    ro.capture_episode(scripted=True, **kw)
    outs = []
    for rep in range(2):
        ro.replay_episode(seeds + rep, guesses)
        g = snap()
        epoch = ro.g_epoch.clone()
        runs = []
        for dual in (True, False):                   # the value base's forwards on the second stream, and on the main stream
            ro.dual_stream = dual
            ro.sample_step = 0
            ro.run_episode(seeds + rep, scripted_guesses=guesses, epoch=epoch, **kw)
            runs.append(snap())
        ro.dual_stream = True
        for k in g:
            assert torch.equal(g[k], runs[0][k]) and torch.equal(runs[0][k], runs[1][k]), (rep, k)
        outs.append(g)
    assert int(outs[0]["n_steps"].sum()) > 3 * B and not torch.equal(outs[0]["tokens"], outs[1]["tokens"])
    # lanes: greedy episodes are noise-independent — one lane and two lanes in flight give the same batches
    kw = dict(temperature=0.0, sample_seed=3, use_graph=True)
    one, s1 = ro.text_env_eval(4 * B, seed_generator=iter(range(100, 10 ** 6)), **kw)
    two, s2 = ro.text_env_eval(4 * B, seed_generator=iter(range(100, 10 ** 6)), concurrent=2, **kw)
    assert len(one) == 4 * B and one == two and s1 == s2
    assert ro._lanes[1][0].qh[0].data_ptr() != ro.qh[0].data_ptr() and ro._lanes[1][0]._qh_ws.data_ptr() != ro._qh_ws.data_ptr()
    ro.close()


class _CharTok:
    """Deterministic stand-in tokenizer: one token per character."""
    def __init__(self, vocab):
        self.vocab, self.pad_token_id, self.eos_token_id = vocab, vocab - 1, 10   # '\n'

    def encode(self, s):
        return [ord(c) % (self.vocab - 1) for c in s]

    def decode(self, ids):
        return "".join(chr(i) for i in ids)


def _oracle_greedy(sd, cfg, prompt_ids, max_new, eos, extra_logits=None, margin=1e-3):
    from oracle import gpt2 as O
    ids, out = list(prompt_ids), []
    for _ in range(max_new):
        lg = O.forward(sd, torch.tensor([ids]), cfg.n_head)[0, -1, : cfg.vocab]
        if extra_logits is not None:
            lg = lg + extra_logits(ids)
        top2 = lg.topk(2)
        if top2.values[0] - top2.values[1] <= margin:
            return out, False
        t = int(top2.indices[0]); ids.append(t); out.append(t)
        if t == eos:
            break
    return out, True


@pytest.mark.parametrize("matmul", ["f32", "bf16x3"])
def test_text_policies_on_f32_engines_reuse_the_prefix_and_match_the_oracle(dev, matmul):
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    from lmrl_gym_amd.policies import GPT2PPOPolicy, GPT2ValuePolicy, heads_to_engine_layout
    from oracle import gpt2 as O, rl
    cfg = GPT2Config(2, 2, 128, 256, 130, 96)
    mk = lambda seed: {k: (v * 6 if v.dim() == 2 else v) for k, v in init_hf_style_state_dict(cfg, seed=seed).items()}
    sd, sd_v = mk(21), mk(22)
    pi, vb = GPT2EngineF32(cfg, sd, dev, matmul=matmul), GPT2EngineF32(cfg, sd_v, dev, matmul=matmul)
    tok = _CharTok(cfg.vocab)
    d, V, beta = cfg.d_model, cfg.vocab, 3.0
    h1, h2 = _mlp_params(d, V, 31, w2_scale=0.2), _mlp_params(d, V, 32, w2_scale=0.2)
    lay = lambda hp: heads_to_engine_layout(hp, cfg.vocab_padded, dev, engine=pi)

    def extra(ids):
        _, hid = O.forward(sd_v, torch.tensor([ids]), cfg.n_head, return_hidden=True)
        q = [rl.mlp_head(hid[0, -1], p["dense1.kernel"], p["dense1.bias"], p["dense2.kernel"], p["dense2.bias"]) for p in (h1, h2)]
        return rl.value_rl_logits(None, q[0], q[1], beta)

    margin = 1e-3 if matmul == "f32" else 2e-2
    common = dict(max_input_length=48, max_new_tokens=5, do_sample=False, eos_token_id=tok.eos_token_id)
    for pol, ex in ((GPT2ValuePolicy(pi, vb, lay(h1), lay(h2), beta, tok, **common), extra), (GPT2PPOPolicy(pi, tok, **common), None)):
        hists = [(E.Text("Wordle:\n", False),), (E.Text("abc def\n", False), E.Text("go\n", True), E.Text("hm\n", False))]
        n_ok, prev = 0, None
        for call in range(2):
            res = pol.act(hists, [False, False])
            if call == 1:           # the second call forwards only what follows the previous prompt (set_len keeps the common prefix)
                assert pol._gen.prefilled_tokens - prev < sum(len(tok.encode(E.text_history_to_str(h))) for h in hists)
            prev = pol._gen.prefilled_tokens
            for h, r in zip(hists, res):
                exp, ok = _oracle_greedy(sd, cfg, tok.encode(E.text_history_to_str(h)), 5, tok.eos_token_id, extra_logits=ex, margin=margin)
                assert r[-1].text == tok.decode(exp) if ok else r[-1].text.startswith(tok.decode(exp)), (type(pol).__name__, call)
                n_ok += len(exp)
            hists = [tuple(r) + (E.Text("ok\n", False),) for r in res]
        assert n_ok >= 4, (type(pol).__name__, n_ok)


def test_f32_value_head_top_k_top_p_match_the_oracle_warpers(dev):
    from lmrl_gym_amd import jax_prng as JP
    from lmrl_gym_amd.gpt2 import RNG_JAX, GPT2Config, SampleParams, init_hf_style_state_dict
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    from lmrl_gym_amd.policies import heads_to_engine_layout
    from oracle import jax_random as JR, rl, warpers as OW
    cfg = GPT2Config(1, 2, 128, 256, 5000, 128)
    sd = init_hf_style_state_dict(cfg, seed=8)
    sd["wte.weight"] = sd["wte.weight"] * 5
    eng = GPT2EngineF32(cfg, sd, dev, matmul="f32")
    B, d, V, beta = 256, cfg.d_model, cfg.vocab, 2.0
    hp1, hp2 = _mlp_params(d, V, 41), _mlp_params(d, V, 42)
    l1, l2 = (heads_to_engine_layout(hp, cfg.vocab_padded, dev, engine=eng) for hp in (hp1, hp2))
    g = torch.Generator().manual_seed(9)
    h = torch.randn(B, d, generator=g)
    ses = eng.session(B, 16)
    qh = [eng.q_hidden_buffer(B) for _ in range(2)]
    hd = h.to(dev)
    for i, head in enumerate((l1, l2)):
        eng.q_hidden(head, hd, qh[i])
    q = [rl.mlp_head(h.double(), *(hp[k] for k in ("dense1.kernel", "dense1.bias", "dense2.kernel", "dense2.bias"))) for hp in (hp1, hp2)]
    z = rl.value_rl_logits(h.double() @ sd["wte.weight"][:V].double().t(), q[0], q[1], beta).numpy()
    key = JR.prng_key(77)
    checked = 0
    for top_k, top_p in ((40, 0.0), (0, 0.95), (40, 0.95)):
        key, sub = JR.split(key)
        p = SampleParams(1.0, top_k, JP.key_to_seed(tuple(int(x) for x in sub)), 0, 0.0, beta, cfg.vocab, None, top_p, RNG_JAX)
        tok, _ = ses.sample(p, hidden=hd, q1=(qh[0], l1["w2"], l1["b2"]), q2=(qh[1], l2["w2"], l2["b2"]), want_logprob=False)
        got = tok.cpu().numpy()
        zs, keep = OW.warp(z, 1.0, top_k, top_p)
        noise = JR.gumbel(sub, (B, V)).astype(np.float64)
        for b in range(B):
            srt = np.sort(zs[b])[::-1]
            if top_k and srt[top_k - 1] - srt[top_k] < 1e-3:
                continue                                         # the k-th / (k+1)-th boundary inside fp32 noise
            if top_p:
                zk = np.where(OW.warp(z[b:b + 1], 1.0, top_k, 0.0)[1][0], zs[b], -np.inf)
                pr = np.sort(np.exp(zk - zk.max()))[::-1]
                pr = pr / pr.sum()
                if np.abs(np.cumsum(pr) - top_p).min() < 2e-5:
                    continue                                     # the nucleus' crossing inside fp32 noise
            sc = np.where(keep[b], zs[b] + noise[b], -np.inf)
            t2 = np.partition(sc, -2)[-2:]
            if t2[1] - t2[0] < 1e-3:
                continue
            checked += 1
            assert int(sc.argmax()) == int(got[b]), (top_k, top_p, b)
    print(f"warpers: {checked} of {3 * B} draws outside the margins")
    assert checked >= 0.6 * 3 * B, checked


def test_mixed_engines_and_head_layouts_are_refused(dev):
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.envs import wordle as W
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine, init_hf_style_state_dict
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    from lmrl_gym_amd.policies import GPT2ValuePolicy, heads_to_engine_layout
    from lmrl_gym_amd.rollout import WordleRolloutEngine
    cfg = GPT2Config(1, 2, 128, 256, 50257, 128)
    sd = init_hf_style_state_dict(cfg, seed=5)
    bf, f32, x3 = GPT2Engine(cfg, sd, dev), GPT2EngineF32(cfg, sd, dev, matmul="f32"), GPT2EngineF32(cfg, sd, dev, matmul="bf16x3")
    hp = _mlp_params(cfg.d_model, cfg.vocab, 1)
    lay = {e: heads_to_engine_layout(hp, cfg.vocab_padded, dev, engine=e) for e in (bf, f32, x3)}
    assert lay[bf]["w2"].dtype == torch.bfloat16 and lay[f32]["w2"].dtype == torch.float32 and "w2_x3" in lay[x3]
    assert torch.equal(lay[bf]["w2"], heads_to_engine_layout(hp, cfg.vocab_padded, dev)["w2"])
    assert torch.equal(lay[f32]["w2"][: cfg.vocab], hp["dense2.kernel"].t().to(dev)) and not lay[f32]["w2"][cfg.vocab:].any()
    vocab = W.Vocabulary.builtin("wordle_official_400.txt")
    tok = _CharTok(cfg.vocab)
    bad = [(bf, f32, lay[bf]), (f32, bf, lay[f32]), (f32, x3, lay[f32]), (x3, f32, lay[x3]), (f32, f32, lay[bf]), (f32, f32, lay[x3]),
           (x3, x3, lay[f32]), (bf, bf, lay[f32])]
    for pi, vb, head in bad:
        with pytest.raises(_lib.LmrlError):
            WordleRolloutEngine(pi, vocab, 8, value_engine=vb, q1_head=head, q2_head=head, beta=1.0)
        with pytest.raises(_lib.LmrlError):
            GPT2ValuePolicy(pi, vb, head, None, 1.0, tok)
    for e in (bf, f32, x3):                       # the matching combinations build
        WordleRolloutEngine(e, vocab, 8, value_engine=e, q1_head=lay[e], q2_head=None, beta=1.0).close()


@pytest.mark.parametrize("device_rollouts", ["0", "1"])
def test_harness_ilql_evaluates_on_the_f32_engine(tmp_path, device_rollouts):
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("harness", os.path.join(os.path.dirname(__file__), "..", "scripts", "harness.py"))
    H = importlib.util.module_from_spec(spec); spec.loader.exec_module(H)
    data = str(tmp_path / "d.jsonl")
    H.main(["gen-data", "--n-data", "24", "--out", data, "--prob-smart", "0.6"])
    H.main(["ilql", "--train-data", data, "--epochs", "1", "--max-steps", "1", "--train-bsize", "8", "--max-length", "80", "--policy-n-rollouts", "4",
            "--policy-bsize", "4", "--policy-max-input-length", "88", "--policy-max-output-length", "8", "--beta", "4",
            "--device-rollouts", device_rollouts, "--policy-engine", "f32"])
