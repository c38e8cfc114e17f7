"""GPU tier: the device-resident Twenty Questions rollout loop (`lmrl_gym_amd.tq_rollout.TwentyQuestionsRolloutEngine`, csrc/tq_tokens.hip) against
the generic text path it replaces (`BatchedTwentyQuestionsPolicyEnvironment(GPT2EngineOracle)` + `GPT2PPOPolicy` + `interact_environment`), its
graph replay against eager launches, its host re-judgement, and its PPO records against the chains of the PPO script
(llm_rl_scripts/twenty_questions/ppo/train_ppo.py:312-352, twenty_questions/env/{env,data,oracle}.py)."""
import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu

NL = 10
MAX_IN, OMAX_IN = 128, 200


def osp(x):
    return x.removesuffix("\n") + "\n"


@pytest.fixture(autouse=True)
def rule_tagger():
    from lmrl_gym_amd.envs import twenty_questions as TQ
    TQ.set_pos_tagger(TQ.rule_pos_tag)
    yield
    TQ.set_pos_tagger(None)


def _weights(vocab, seed, alphabet, boost=1.0, pos_scale=16.0):
    """Random tiny GPT-2 weights that spell context-dependent strings from `alphabet` under greedy decoding: the final layer norm's bias adds exactly
    `boost` to the (tied) LM head's logit of every alphabet id — above what a random model's own logits reach (std 0.02 sqrt(d)) — and the position
    embeddings are scaled up (the other ids' embeddings down), so that the winner among the alphabet changes with the position and the history's length instead of repeating the last
    token (whose embedding is otherwise the largest part of its own hidden state)."""
    import torch
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    cfg = GPT2Config(2, 2, 128, 256, vocab, 256)
    sd = init_hf_style_state_dict(cfg, seed=seed)
    ids = [ord(c) for c in alphabet]
    keep = torch.zeros(vocab, 1)
    keep[ids] = 1.0
    sd["wte.weight"] = sd["wte.weight"] * (0.05 + 0.95 * keep)           # every other id: a faint embedding, hence a logit near 0
    w = sd["wte.weight"][ids].double()
    sd["ln_f.bias"] = (w.T @ torch.linalg.solve(w @ w.T, torch.full((len(alphabet),), float(boost), dtype=torch.float64))).float()
    sd["wpe.weight"] = sd["wpe.weight"] * pos_scale
    return cfg, sd


def _engine(cfg, sd, dev, kind):
    from lmrl_gym_amd.gpt2 import GPT2Engine
    if kind == "bf16":
        return GPT2Engine(cfg, sd, dev)
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    return GPT2EngineF32(cfg, sd, dev, matmul=kind)


def _pair(dev, kind, seed=0):
    from lmrl_gym_amd.datasets import ByteTokenizer
    tok = ByteTokenizer()
    cfg, sd = _weights(len(tok) + 3, seed, "Isitacdogbrne ?\n")
    ocfg, osd = _weights(len(tok) + 3, seed + 100, "yesnoYN .\n")
    return tok, _engine(cfg, sd, dev, kind), _engine(ocfg, osd, dev, kind), (cfg, sd)


def _env(T, B=None, oracle=None):
    from lmrl_gym_amd.envs import twenty_questions as TQ
    return TQ.BatchedTwentyQuestionsPolicyEnvironment(oracle, TQ.get_default_word_list(), max_conversation_length=T, bsize=B)


@pytest.mark.parametrize("kind,B", [("bf16", 8), ("bf16", 33), ("f32", 8), ("f32", 33)])
def test_greedy_device_loop_equals_generic_text_path(kind, B):
    """Same two models, greedy decoding, per-env seeds (some in deterministic mode): the device loop's transitions — texts, rewards, dones — equal
    `interact_environment(BatchedTwentyQuestionsPolicyEnvironment(GPT2EngineOracle), GPT2PPOPolicy)`; the episodes end by the question budget."""
    import torch
    from lmrl_gym_amd import _lib, environment as E
    from lmrl_gym_amd.envs import twenty_questions as TQ
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
    dev = _lib.require_gpu()
    tok, eng, oeng, _ = _pair(dev, kind)
    T, G = 4, 9
    seeds = [3 + 7 * b if b % 5 else 2 ** 40 + b for b in range(B)]
    options = [dict(deterministic=True) if b % 3 == 1 else None for b in range(B)]
    ro = TwentyQuestionsRolloutEngine(eng, oeng, tok, _env(T), B, G, NL, MAX_IN, OMAX_IN)
    plain = TwentyQuestionsRolloutEngine(eng, oeng, tok, _env(T), B, G, NL, MAX_IN, OMAX_IN, reuse_generated=False)
    assert ro.judge == "device"
    # every env starts from the same history and a greedy guesser asks them all the same question until the answers differ: once with the
    # oracle model's own answers, once with answers injected on both sides (the oracle model still runs), so that the histories fan out
    codes = np.array([[(b * 5 + t * 3 + b // 4) % 2 for t in range(T)] for b in range(B)], dtype=np.int8)
    kept = 0
    for scripted in (False, True):
        ro.set_scripted_answers(codes if scripted else None)
        ro.run_episode(seeds, options, temperature=0.0, use_graph=True, sync_every=0)
        torch.cuda.synchronize()
        mine, recs = ro.interactions(), ro.records()
        oracle = ScriptedOracle(codes) if scripted else TQ.GPT2EngineOracle(oeng, tok, max_input_length=OMAX_IN, max_new_tokens=4, eos_token_id=NL)
        env = _env(T, B, oracle)
        pol = GPT2PPOPolicy(eng, tok, max_input_length=MAX_IN, max_new_tokens=G, do_sample=False, eos_token_id=NL, out_str_process=osp)
        ref = E.interact_environment(env, pol, env_seed=seeds, env_options=options, bsize=B)
        assert [r["word"] for r in recs] == [int(i) for i in env._games.word_idx]
        n_steps = 0
        for b, (x, y) in enumerate(zip(mine, ref)):
            assert len(x) == len(y), (b, len(x), len(y))
            for i, (tx, ty) in enumerate(zip(x, y)):
                assert tx == ty, (b, i, tx, ty)
                n_steps += 1
        for b, r in enumerate(recs):                    # the device's own text is the host's decoding of the same ids
            assert [q.decode("utf-8") for q in r["question"]] == [t.post_action_history[-1].text for t in mine[b]], b
        texts = {t.post_action_history[-1].text for ep in mine for t in ep}
        answers = np.concatenate([r["answer"] for r in recs])
        ogen = {tuple(g) for r in recs for g in r["ogen"]}
        print(f"[20q greedy {kind} B={B} scripted={scripted}] transitions={n_steps} distinct questions={len(texts)} {sorted(texts)[:4]} "
              f"yes={int(answers.sum())}/{len(answers)} distinct oracle outputs={len(ogen)}")
        assert n_steps >= B and len(texts) >= (4 if scripted else 2) and any(len(x.strip()) >= 3 for x in texts) and len(ogen) >= 2
        assert any(len(ep) == T and ep[-1].done and ep[-1].reward == -1.0 for ep in mine)
        # the other schedule of the guesser's cache — every question forwarded again from its canonical ids — gives the same transitions
        plain.set_scripted_answers(codes if scripted else None)
        plain.run_episode(seeds, options, temperature=0.0, use_graph=scripted, sync_every=0)
        assert plain.interactions() == mine
        fwd = [int(x) for x in (ro.traj["feed_start"].cpu() - plain.traj["feed_start"].cpu()).tolist()]
        assert min(fwd) >= 0                            # (the last turn's feed: `ro` kept generated rows that `plain` forwarded again)
        kept += max(fwd)
    assert kept > 0
    ro.close()
    plain.close()


class ScriptedOracle:
    """The host env's oracle for the replay: slot b's answer in turn t is codes[b][t]."""

    def __init__(self, codes):
        self.codes, self.turn = codes, 0

    def generate_answers(self, words, questions, return_full=False):
        from lmrl_gym_amd.envs.twenty_questions import INVALID_QUESTION
        out = ["No." if q == INVALID_QUESTION else ("Yes." if self.codes[b][self.turn] else "No.") for b, q in enumerate(questions)]
        self.turn += 1
        return out


def _thing_tagger(text):
    """A tagger that is not the stand-in: it does not take "thing" for a noun."""
    from lmrl_gym_amd.envs.twenty_questions import rule_pos_tag
    return [(t, "DT" if t == "thing" else tag) for t, tag in rule_pos_tag(text)]


# per env: (seed, [(question, answer code)] per turn); deterministic mode, word = seed: 10 Cat, 11 Dog, 12 Horse
_PLANS = [
    (10, [("is it big?", 0), ("a cat?", 1)]),                                       # ends by a guess in turn 2
    (11, [("a cat?", 1), ("a dog", 0), ("is it a dog?", 1)]),                       # an affirmed question that does not name the word; a guess of 12 ids:
                                                                                    #   no room for the newline, the canonical ids differ from the generated
    (10, [("a cat\xa0?", 1), ("x", 1)]),                                            # affirmed, non-ASCII, naming: the host ends the game here
    (10, [("a c\xe4t?", 1), ("a d\xf6g?", 1), ("cat", 0), ("Cat!! 7", 1)]),         # affirmed non-ASCII questions that do not name it
    (12, [("a horse", 0), ("", 1), ("\t horse \x1f", 1)]),                          # an empty question; blanks of both kinds around a guess
    (11, [("thing a dog", 1)]),                                                     # the taggers disagree about this one
    (12, [("is it?", 1), ("is it?", 1), ("is it?", 1), ("is it?", 1)]),             # affirmed to the budget
]


@pytest.mark.parametrize("tagger,judge", [("rule", "auto"), ("thing", "host")])
def test_steered_games_equal_the_env_and_flagged_turns_are_rejudged_on_the_host(tagger, judge):
    """Forced questions (the steered sampler) with scripted answers, then the device's OWN decoded question texts fed turn by turn to
    `BatchedTwentyQuestionsPolicyEnvironment` with an oracle that gives the same answers: histories, rewards, dones and episode lengths equal.
    Covers a guess, an affirmed non-naming question, affirmed non-ASCII questions (the post-hoc cut, and none), questions whose generation is not
    their canonical encoding; with an injected tagger that differs from the stand-in (judge = "host") every affirmed question is the host's."""
    import torch
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.environment import Text
    from lmrl_gym_amd.envs import twenty_questions as TQ
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
    dev = _lib.require_gpu()
    if tagger == "thing":
        TQ.set_pos_tagger(_thing_tagger)
    tok, eng, oeng, _ = _pair(dev, "bf16")
    T, G, B = 4, 12, len(_PLANS) + 2
    plans = _PLANS + [(20 + b, [("is it?", b % 2)]) for b in range(2)]
    seeds = [p[0] for p in plans]
    options = [dict(deterministic=True)] * B
    pad = lambda qa: list(qa) + [("zz", 0)] * (T - len(qa))
    script = [pad(p[1]) for p in plans]
    ro = TwentyQuestionsRolloutEngine(eng, oeng, tok, _env(T), B, G, NL, MAX_IN, OMAX_IN, judge=judge)
    assert ro.judge == ("device" if tagger == "rule" else "host")
    ro.set_scripted_questions([[script[b][t][0] for b in range(B)] for t in range(T)], strength=60.0)
    codes = np.array([[script[b][t][1] for t in range(T)] for b in range(B)], dtype=np.int8)
    ro.set_scripted_answers(codes)
    ro.run_episode(seeds, options, temperature=0.0, use_graph=True, sync_every=0)
    torch.cuda.synchronize()
    raw_turns = ro.traj["n_turns"].cpu().numpy().copy()
    recs, inter = ro.records(), ro.interactions()
    # ---- the steering worked
    for b in range(B):
        for t, tr in enumerate(inter[b]):
            assert tr.post_action_history[-1].text == osp((script[b][t][0] + "\n").encode("utf-8")[:G].decode("utf-8")), (b, t)
    # ---- the device's own texts through the env
    env = _env(T, B, ScriptedOracle(codes))
    hist = env.reset(seeds, options)
    assert [r["word"] for r in recs] == [int(i) for i in env._games.word_idx] == [s % len(env.word_list) for s in seeds]
    done = [False] * B
    for t in range(T):
        if all(done):
            break
        for b in range(B):
            assert (len(inter[b]) > t) == (not done[b]), (b, t)
        acts = [tuple(hist[b]) + (inter[b][t].post_action_history[-1],) if not done[b] else None for b in range(B)]
        out = env.step(acts, list(done))
        for b in range(B):
            if done[b]:
                continue
            tr = inter[b][t]
            assert tr.pre_action_history == tuple(hist[b]) and tr.post_action_history == acts[b], (b, t)
            nh, r, d = out[b]
            assert tr.post_transition_history == tuple(nh) and tr.reward == r and tr.done == d, (b, t, tr, out[b])
            assert isinstance(tr.post_action_history[-1], Text) and tr.post_action_history[-1].is_action
            hist[b], done[b] = nh, d
    assert all(done)
    lens = [len(ep) for ep in inter]
    assert lens[0] == 2 and inter[0][-1].reward == 0.0 and inter[0][-1].done                  # the guess
    assert lens[1] == 3 and inter[1][0].reward == -1.0 and inter[1][-1].reward == 0.0         # affirmed without naming, then the 12-id guess
    assert lens[2] == 1 and inter[2][0].reward == 0.0 and raw_turns[2] == T                   # cut on the host: the device had played on
    assert lens[3] == 4 and [t.reward for t in inter[3]] == [-1.0, -1.0, -1.0, 0.0]
    assert lens[4] == 3 and inter[4][1].post_action_history[-1].text == "\n" and inter[4][-1].reward == 0.0
    assert lens[5] == (1 if tagger == "thing" else 4)                                         # only the injected tagger takes it for a guess
    assert lens[6] == 4 and inter[6][-1].done and inter[6][-1].reward == -1.0                 # the budget
    flags = [r["flag"].tolist() for r in recs]
    if tagger == "rule":
        assert flags[2] == [True] and flags[3] == [True, True, False, False] and not any(flags[0]) and not any(flags[1])
    else:
        assert all(f == bool(a) for r in recs for f, a in zip(r["flag"], r["answer"]))
        assert raw_turns[0] == T and raw_turns[5] == T                                        # nothing ended on the device but by the budget
    ro.close()


def _snapshot(ro):
    import torch
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy().copy() for k, v in ro.traj.items()}
    nt = h["n_turns"]
    live = np.arange(ro.T)[None, :] < nt[:, None]
    out = dict(n_turns=nt, ep_reward=h["ep_reward"], word=h["word"])
    for k in ("gen_len", "q_len", "ogen_len", "answer", "reward", "done", "flag"):
        out[k] = np.where(live, h[k], 0)
    for k, ln in (("gen", "gen_len"), ("q_text", "q_len"), ("ogen", "ogen_len")):
        m = live[:, :, None] & (np.arange(h[k].shape[2])[None, None, :] < h[ln][:, :, None])
        out[k] = np.where(m, h[k], 0)
    out["hist"] = np.where(np.arange(h["hist"].shape[1])[None, :] < h["hist_len"][:, None], h["hist"], 0)
    return out


def test_graph_replay_equals_eager_and_two_engines_do_not_disturb_each_other():
    """Sampled episodes: graph replay == eager launches bit for bit; two engines with different weights, their episodes interleaved, each reproduce
    their own record; another episode number draws other questions."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
    dev = _lib.require_gpu()
    B, T, G = 24, 3, 8
    seeds = list(range(100, 100 + B))
    ros = []
    for s in (0, 5):
        tok, eng, oeng, _ = _pair(dev, "bf16", seed=s)
        ros.append(TwentyQuestionsRolloutEngine(eng, oeng, tok, _env(T), B, G, NL, MAX_IN, OMAX_IN))
    kw = dict(temperature=1.0, sample_seed=(7 << 32) | 12345, episode=3, sync_every=0)
    eager = []
    for ro in ros:
        ro.run_episode(seeds, None, use_graph=False, **kw)
        eager.append(_snapshot(ro))
    assert not np.array_equal(eager[0]["gen"], eager[1]["gen"])
    for _ in range(2):                                  # a, b, a, b: the second round replays graphs captured before the other engine ran
        for ro, want in zip(ros, eager):
            ro.run_episode(seeds, None, use_graph=True, **kw)
            got = _snapshot(ro)
            for k in want:
                assert np.array_equal(want[k], got[k]), k
    ros[0].run_episode(seeds, None, use_graph=True, **dict(kw, episode=4))
    assert not np.array_equal(_snapshot(ros[0])["gen"], eager[0]["gen"])
    # the warpers (the sampler's materialised-logits operand): graph == eager, and top_k = 1 is greedy decoding
    for warp in (dict(top_k=5), dict(top_p=0.8), dict(top_k=8, top_p=0.9)):
        snaps = []
        for graph in (False, True):
            ros[0].run_episode(seeds, None, use_graph=graph, **kw, **warp)
            snaps.append(_snapshot(ros[0]))
        for k in snaps[0]:
            assert np.array_equal(snaps[0][k], snaps[1][k]), (warp, k)
        assert not np.array_equal(snaps[0]["gen"], eager[0]["gen"]), warp
    ros[0].run_episode(seeds, None, use_graph=True, **kw, top_k=1)
    top1 = _snapshot(ros[0])
    ros[0].run_episode(seeds, None, use_graph=True, **dict(kw, temperature=0.0))
    greedy = _snapshot(ros[0])
    for k in top1:
        assert np.array_equal(top1[k], greedy[k]), k
    assert (eager[0]["gen_len"] > 0).any()
    for ro in ros:
        ro.close()


@pytest.mark.parametrize("matmul", ["f32", "bf16"])
def test_tq_ppo_records_and_device_ppo_data_equal_the_host_chain_path(matmul):
    """`ppo_records()` == `PPORecords.from_token_trajectory_chains` of the chains the PPO script's loop builds from the same interactions (one
    trajectory per episode, the whole history, the reward on each question's last token); `ppo_data` == the host form at the tolerances of
    tests/test_gpu_ppo_device.py's chess / Maze twins; the drop-the-last-turns rule is applied when `max_length` is within reach."""
    import sys
    import os
    import torch
    from lmrl_gym_amd import _lib, environment as E
    from lmrl_gym_amd.algorithms import ppo
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ppo_device import PPORecords, ppo_data_from_records
    from lmrl_gym_amd.algorithms.ppo_inference import GPT2PPOInference
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, LinearHeadF32
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import rl as ORL
    dev = _lib.require_gpu()
    tok, eng, oeng, (cfg, sd) = _pair(dev, "bf16", seed=2)
    B, T, G = 20, 4, 10
    ro = TwentyQuestionsRolloutEngine(eng, oeng, tok, _env(T), B, G, NL, MAX_IN, OMAX_IN)
    plans = [_PLANS[b % len(_PLANS)] for b in range(B)]
    ro.set_scripted_questions([[(plans[b][1] + [(None, 0)] * T)[t][0] for b in range(B)] for t in range(T)], strength=12.0)
    ro.set_scripted_answers(np.array([[(plans[b][1] + [(None, -1)] * T)[t][1] for t in range(T)] for b in range(B)], dtype=np.int8))
    ro.run_episode([p[0] for p in plans], dict(deterministic=True), temperature=1.0, sample_seed=8, use_graph=False, sync_every=0)
    torch.cuda.synchronize()
    inter = ro.interactions()
    assert len({len(ep) for ep in inter}) >= 2
    chains = []
    for ep in inter:                                    # twenty_questions/ppo/train_ppo.py:322-352
        tt = E.TextTrajectory(ep[-1].post_transition_history, tuple(sum([[t.reward, 0.0] for t in ep], [0.0])), ep[-1].done)
        chains.append(E.TokenTrajectoryChain(E.TokenTrajectory.from_text_trajectory(tt, tok), None))
    rec, want = ro.ppo_records(), PPORecords.from_token_trajectory_chains(chains, device=dev)
    assert rec.chain is None and rec.n == rec.n_chains == B
    g, w = ({k: getattr(r, k).cpu().numpy() for k in ("tokens", "is_action", "reward", "n_tok", "done")} for r in (rec, want))
    assert np.array_equal(g["n_tok"], w["n_tok"]) and np.array_equal(g["done"].astype(bool), w["done"].astype(bool))
    for b in range(B):
        n = int(g["n_tok"][b])
        for k in ("tokens", "is_action", "reward"):
            assert np.array_equal(g[k][b, :n], w[k][b, :n]), (b, k)
    assert len(set(g["n_tok"].tolist())) >= 2 and (g["reward"] == -1.0).any() and g["done"].any()
    gen = torch.Generator().manual_seed(6)
    sd2 = {kk: v + 0.02 * torch.randn(v.shape, generator=gen) * v.abs().mean().clamp_min(1e-3) for kk, v in sd.items()}
    pol, init = GPT2F32(sd2, cfg.n_head, device=dev, matmul=matmul), GPT2F32(sd, cfg.n_head, device=dev, matmul=matmul)
    tol = 1e-5 if matmul == "f32" else 2e-3            # tests/test_gpu_ppo_device.py: the two forms run the same bf16 products on different paddings
    vh = LinearHeadF32(dict(kernel=torch.randn(cfg.d_model, 1, generator=gen) * 0.05, bias=torch.tensor([0.2])), dev)
    inf = GPT2PPOInference(pol, vh, tok.pad_token_id, initial_policy=init)
    kw = dict(gamma=0.97, lam=0.9, kl_weight=0.05)

    def compare(ds, kls, host_chains, max_length):
        datas, kls_h = inf.get_ppo_data_from_token_trajectory_chain(host_chains, bsize=32, max_length=max_length, **kw)
        host = ppo.PPODataset.from_ppo_data_list(datas, tok, BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, max_length))
        got = ds.to_host()
        assert (got.input_ids == host.input_ids).all() and (got.should_take_action == host.should_take_action).all()
        np.testing.assert_allclose(got.old_logprobs, host.old_logprobs, rtol=0, atol=tol)
        np.testing.assert_allclose(got.old_values, host.old_values, rtol=0, atol=tol)
        np.testing.assert_allclose(got.old_returns, host.old_returns, rtol=tol, atol=tol)
        np.testing.assert_allclose(got.old_advantages, host.old_advantages, rtol=2 * tol, atol=2 * tol)
        np.testing.assert_allclose(kls.cpu().numpy(), kls_h, rtol=1e-5 if matmul == "f32" else 5e-2, atol=5e-6 if matmul == "f32" else 2e-4)
    max_length = int(g["n_tok"].max()) + 1              # out of reach: nothing is dropped
    ds, kls = ro.ppo_data(inf, max_length=max_length, bsize=64, **kw)
    assert ro.last_truncation == dict(shortened=0, skipped=0)
    compare(ds, kls, chains, max_length)
    # ---- within reach: the script's loop on the host records (restated in oracle/rl.py) gives the chains the device rule must produce
    max_length = int(np.sort(g["n_tok"])[B // 2])
    kept = [ORL.truncate_turns_record(dict(tokens=g["tokens"][b, :g["n_tok"][b]], is_action=g["is_action"][b, :g["n_tok"][b]].astype(bool),
                                           reward=g["reward"][b, :g["n_tok"][b]], done=bool(g["done"][b])), max_length, kw["gamma"]) for b in range(B)]
    kept = [k for k in kept if k is not None]
    short = [E.TokenTrajectoryChain(E.TokenTrajectory(np.asarray(k["tokens"], dtype=np.int32), np.asarray(k["is_action"], dtype=bool),
                                                      np.asarray(k["reward"], dtype=np.float32), np.asarray(bool(k["done"]))), None) for k in kept]
    ds, kls = ro.ppo_data(inf, max_length=max_length, bsize=64, **kw)
    assert ro.last_truncation["shortened"] > 0 and ro.last_truncation["skipped"] == B - len(kept)
    compare(ds, kls, short, max_length)
    ro.close()


def test_ppo_rollouts_equals_the_round_done_by_hand():
    """`ppo_rollouts` over two episode batches, the last one partial (B = 8, 11 rollouts: idle envs, the concat, ONE whitening over the round) ==
    the same round done by hand on an identically built engine — per batch `run_episode(n_live=actual)` + `ppo_data(n=actual,
    use_advantage_whitening=False)`, then `DevicePPODataset.concat` and one `dist.whiten_distributed` over the action tokens — bit for bit (both
    sides run the same kernels on the same inputs); `summary` is mean / std / min / max of the records' `ep_reward`, last `done` and `n_turns`."""
    import itertools
    import torch
    from lmrl_gym_amd import _lib, dist as D
    from lmrl_gym_amd.algorithms.ppo_device import DevicePPODataset
    from lmrl_gym_amd.algorithms.ppo_inference import GPT2PPOInference
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, LinearHeadF32
    dev = _lib.require_gpu()
    tok, eng, oeng, (cfg, sd) = _pair(dev, "bf16", seed=2)
    B, T, G, N = 8, 4, 12, 11
    plans = [_PLANS[b % len(_PLANS)] for b in range(B)]
    questions = [[(plans[b][1] + [(None, 0)] * T)[t][0] for b in range(B)] for t in range(T)]
    answers = np.array([[(plans[b][1] + [(None, -1)] * T)[t][1] for t in range(T)] for b in range(B)], dtype=np.int8)
    ros = []
    for _ in range(2):
        ro = TwentyQuestionsRolloutEngine(eng, oeng, tok, _env(T), B, G, NL, MAX_IN, OMAX_IN)
        ro.set_scripted_questions(questions, strength=60.0)
        ro.set_scripted_answers(answers)
        ros.append(ro)
    gen = torch.Generator().manual_seed(6)
    sd2 = {kk: v + 0.02 * torch.randn(v.shape, generator=gen) * v.abs().mean().clamp_min(1e-3) for kk, v in sd.items()}
    pol, init = GPT2F32(sd2, cfg.n_head, device=dev, matmul="bf16"), GPT2F32(sd, cfg.n_head, device=dev, matmul="bf16")
    vh = LinearHeadF32(dict(kernel=torch.randn(cfg.d_model, 1, generator=gen) * 0.05, bias=torch.tensor([0.2])), dev)
    inf = GPT2PPOInference(pol, vh, tok.pad_token_id, initial_policy=init)
    kw = dict(gamma=0.97, lam=0.9, kl_weight=0.05, max_length=ros[0].hist_bound + 1, bsize=64)
    run = dict(temperature=1.0, sample_seed=8)
    seed_gen = lambda: (plans[i % B][0] for i in itertools.count())     # env b plays plan b in every batch (deterministic mode: word = seed)
    options = dict(deterministic=True)
    ds, kls, summary = ros[0].ppo_rollouts(inf, N, seed_gen(), options, **kw, **run)
    # ---- the same round by hand
    ro, sg = ros[1], seed_gen()
    parts, kl_parts, stats = [], [], []
    for k, actual in enumerate((B, N - B)):
        seeds = [0] * B
        seeds[:actual] = [next(sg) for _ in range(actual)]
        ro.run_episode(seeds, options, episode=k, use_graph=True, n_live=actual, **run)
        d, kl = ro.ppo_data(inf, n=actual, use_advantage_whitening=False, **kw)
        parts.append(d); kl_parts.append(kl)
        rec = ro.records()[:actual]
        stats += [(r["ep_reward"], float(r["done"][-1]), len(r["done"])) for r in rec]
        assert int(ro.traj["n_turns"][actual:].sum().item()) == 0           # the idle envs of the partial batch recorded nothing
    want = DevicePPODataset.concat(parts)
    adv = want.old_advantages
    want.old_advantages = D.whiten_distributed(adv.view(-1), want.should_take_action.view(-1), shift_mean=True).view(adv.shape)
    assert len(ds) == len(want) == N
    for name in DevicePPODataset.FIELDS:
        assert torch.equal(getattr(ds, name), getattr(want, name)), name
    assert ds.longest == want.longest and (ds.lengths is None) == (want.lengths is None)
    assert ds.lengths is None or torch.equal(ds.lengths, want.lengths)
    assert torch.equal(kls, torch.cat(kl_parts))
    assert ros[0].episodes == 2 and bool(ds.should_take_action.any()) and float(ds.old_advantages.abs().max()) > 0
    lens = [s[2] for s in stats]
    assert min(lens) < T and max(lens) == T                                  # an episode was won early, another ran to the budget
    summ = lambda x: dict(mean=np.mean(x), std=np.std(x), min=np.min(x), max=np.max(x))
    st = np.asarray(stats, dtype=np.float64).T
    assert summary == dict(reward=summ(st[0].astype(np.float32)), done=summ(st[1].astype(np.float32)), length=summ(st[2].astype(np.int64)))
    for ro in ros:
        ro.close()


def test_engine_refuses_what_is_out_of_scope():
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.envs import twenty_questions as TQ
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
    dev = _lib.require_gpu()
    tok, eng, oeng, (cfg, sd) = _pair(dev, "bf16")

    class Merging(ByteTokenizer):
        def encode(self, s):
            return list(s.replace("es", "\x01").encode("utf-8"))
    mk = lambda **kw: TwentyQuestionsRolloutEngine(**dict(dict(engine=eng, oracle_engine=oeng, tokenizer=tok, env=_env(4), batch=4, max_new_tokens=8, eos_token_id=NL,
                                                               max_input_length=MAX_IN, oracle_max_input_length=OMAX_IN), **kw))
    with pytest.raises(ValueError, match="generic"):
        mk(tokenizer=Merging())                                                      # a merging tokenizer
    with pytest.raises(ValueError, match="generic"):
        mk(env=_env(20))                                                             # 11 + 20 * (8 + 1 + 5) tokens do not fit 128
    with pytest.raises(ValueError, match="generic"):
        mk(oracle_max_input_length=100)                                              # the longest prefix + question + suffix does not fit
    for fn in (TQ.asker_postproc, TQ.asker_postproc_simple, TQ.asker_postproc_filter_repeats):
        with pytest.raises(ValueError, match="asker_postproc"):
            mk(out_str_process=fn)
    with pytest.raises(ValueError, match="one class"):
        mk(oracle_engine=_engine(cfg, sd, dev, "f32"))
    TQ.set_pos_tagger(_thing_tagger)
    with pytest.raises(ValueError, match="rule_pos_tag"):
        mk(judge="device")
    ro = mk(out_str_process=osp)
    assert ro.judge == "host"
    with pytest.raises(ValueError, match="seed"):
        ro.run_episode([None] * 4)
    ro.close()
