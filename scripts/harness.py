"""Task harness: the configurations of the reference's task scripts, composed from this package.

    python scripts/harness.py ilql     --train-data d.jsonl [--eval-data e.jsonl]    # llm_rl_scripts/wordle/ilql/train_ilql_gpt2.py
    python scripts/harness.py ppo      [--bc-data d.jsonl]                           # llm_rl_scripts/wordle/ppo/train_ppo_gpt2.py
    python scripts/harness.py ppo      --env maze --device-rollouts 1                # llm_rl_scripts/maze/ppo/train_ppo_online.py (device-resident loop)
    python scripts/harness.py ppo      --env chess --device-rollouts 1               # llm_rl_scripts/chess/ppo/train_ppo_gpt2_online.py (device-resident loop)
    python scripts/harness.py ilql     --device-data 1 --policy mixture --n-data 1000  # the data played and blocked on the device, device batches
    python scripts/harness.py filtered-bc --device-rollouts 1 --device-data 1        # wordle/online_filtered_bc, every round resident in HBM
    python scripts/harness.py bc-eval                                                # llm_rl_scripts/wordle/bc/eval_bc_gpt2.py
    python scripts/harness.py maze-eval                                              # llm_rl_scripts/maze/bc/fully_observed_bc.py (eval part)
    python scripts/harness.py bc-eval  --model-family gptj --model random:gptj-tiny  # llm_rl_scripts/wordle/bc/eval_bc.py (GPT-J, fp32 engine)
    python scripts/harness.py gen-data --n-data 1000 --out d.jsonl                   # llm_rl_scripts/wordle/misc/data_gen.py
    python scripts/harness.py gen-data --policy optimal --start-word raise --device-loop 1 --out d.jsonl   # scripted policies + loop on the device
    python scripts/harness.py optimal-perf --n 1000                                  # llm_rl_scripts/wordle/misc/optimal_perf.py

Hyper-parameter names and defaults are the reference scripts' own.  Not carried over: tyro, wandb, GCS, mesh-shape flags (one
process per GPU + `torch.distributed.run` instead).  `--model` is a checkpoint directory in the reference layout
(`lmrl_gym_amd.checkpoints`) or `random:<tiny|small|medium>`; the GPT-2 tokenizer is `transformers.AutoTokenizer('gpt2')` when its
files are available, else the Wordle-alphabet adapter (`datasets.WordleTokenizer`).  `--model-family gptj` (bc-eval and maze-eval): `--model` is a GPT-J
checkpoint directory (HF PyTorch, or the reference's flax layout) or `random:gptj-tiny`; every other subcommand and `--device-rollouts 1` refuse it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ILQL_DEFAULTS = dict(epochs=10, max_steps=None, lr=3e-5, weight_decay=0.0, train_bsize=32, grad_accum_steps=1, max_length=512, log_every=256,
                     policy_max_input_length=256, policy_max_output_length=256, policy_do_sample=True, policy_temperature=None,
                     policy_top_p=None, policy_top_k=None, policy_num_beams=1, policy_bsize=32, policy_n_rollouts=32, beta=32.0, polyak_alpha=0.005,
                     hard_update_every=None, gamma=0.99, tau=0.7, cql_weight=0.01, bad_word_reward=-10.0,
                     bf16_activations=False, gradient_checkpointing=False)                                   # train_ilql_gpt2.py:41-117, :369
PPO_DEFAULTS = dict(n_rounds=1, epochs=1, max_steps=None, lr=1e-5, weight_decay=0.0, train_bsize=32, train_bc_bsize=None, grad_accum_steps=None,
                    rollout_bsize=32, n_rollouts=128, ppo_data_bsize=32, max_input_length=512, max_output_length=512, policy_do_sample=True,
                    policy_temperature=None, policy_top_p=None, policy_top_k=None, policy_num_beams=1, gamma=1.0, lam=0.95, use_advantage_whitening=True,
                    init_kl_coef=0.001, kl_target=None, kl_horizon=None, cliprange_value=0.2, cliprange=0.2, value_loss_coef=1.0,
                    bc_loss_weight=1.0, bad_word_reward=-10.0, bf16_activations=False, gradient_checkpointing=False)   # train_ppo_gpt2.py:40-112, :211
FILTERED_BC_DEFAULTS = dict(n_rounds=1, epochs=1, max_steps=None, lr=1e-5, weight_decay=0.0, train_bsize=32, grad_accum_steps=None, rollout_bsize=32,
                            n_rollouts=128, filter_percengage=0.3, bf16_activations=False, gradient_checkpointing=False, max_input_length=512,
                            max_output_length=512, policy_do_sample=True, policy_temperature=None, policy_top_p=None, policy_top_k=None, policy_num_beams=1,
                            bad_word_reward=-10.0)                                    # wordle/online_filtered_bc/train_online_filtered_bc_gpt2.py:40-87
BC_EVAL_DEFAULTS = dict(policy_n_rollouts=32, policy_bsize=1, policy_max_input_length=256, policy_max_output_length=256, policy_do_sample=True,
                        policy_temperature=None, policy_top_p=None, policy_top_k=None, policy_num_beams=1)                         # eval_bc_gpt2.py
MAZE_EVAL_DEFAULTS = dict(maze_name="double_t_maze", describe_function="describe_observation_only_walls", reward_function="standard_reward",
                          last_k=1, max_steps=100, generation_bsize=4, max_input_length=128, max_output_length=8)   # fully_observed_bc.py:230-283


def _add(ap: argparse.ArgumentParser, defaults: dict):
    for k, v in defaults.items():
        flag = "--" + k.replace("_", "-")
        if isinstance(v, bool):
            ap.add_argument(flag, type=lambda s: s.lower() in ("1", "true", "yes"), default=v)
        elif v is None:
            ap.add_argument(flag, type=float, default=None)
        else:
            ap.add_argument(flag, type=type(v), default=v)


def _pdrop(a) -> dict:
    """The GPT2F32 dropout rates of --embd-pdrop / --attn-pdrop / --resid-pdrop (default 0.0 each: no dropout launch anywhere)."""
    return dict(embd_pdrop=a.embd_pdrop, attn_pdrop=a.attn_pdrop, resid_pdrop=a.resid_pdrop)


def _step_keys(a):
    """One dropout key per train step: `--seed` -> jax_prng.prng_key, split once per step (the reference train loops' `prng_key, new_key = split`);
    every key is None while all three rates are 0, so the steps run exactly as they do without the flags."""
    from lmrl_gym_amd import jax_prng
    return jax_prng.StepKeys(jax_prng.prng_key(a.seed) if max(_pdrop(a).values()) > 0 else None)


def _tokenizer(wordle: bool = True):
    from lmrl_gym_amd.datasets import ByteTokenizer, WordleTokenizer
    try:
        from transformers import AutoTokenizer
        tok = AutoTokenizer.from_pretrained("gpt2", local_files_only=True)
        tok.add_special_tokens({"pad_token": "<|pad|>"})
        return tok
    except Exception:
        return WordleTokenizer() if wordle else ByteTokenizer()


def _model_gptj(spec: str, vocab: int):
    """--model-family gptj: `random:gptj-tiny` or a GPT-J checkpoint directory (HF PyTorch layout, or the reference's flax layout)."""
    from lmrl_gym_amd import checkpoints as C
    from lmrl_gym_amd.gptj_f32_engine import GPTJConfig, init_hf_style_gptj_state_dict
    if spec.startswith("random:"):
        sizes = {"gptj-tiny": GPTJConfig(2, 2, 128, 32, 256, vocab, 2048)}
        if spec.split(":")[1] not in sizes:
            raise SystemExit(f"--model-family gptj: --model {spec} is not one of " + ", ".join("random:" + k for k in sizes))
        cfg = sizes[spec.split(":")[1]]
        return cfg, init_hf_style_gptj_state_dict(cfg, seed=0)
    import torch
    loader = C.load_hf_pytorch_gptj if os.path.exists(os.path.join(spec, "model.safetensors")) or os.path.exists(os.path.join(spec, "pytorch_model.bin")) \
        else C.load_gptj_checkpoint
    cfg, sd = loader(spec)
    return cfg, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _model(spec: str, vocab: int, family: str = "gpt2"):
    from lmrl_gym_amd import checkpoints as C
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    if family == "gptj":
        return _model_gptj(spec, vocab)
    if spec.startswith("random:gptj"):
        raise SystemExit(f"--model {spec} needs --model-family gptj")
    if spec.startswith("random:"):
        cfg = dict(tiny=GPT2Config(2, 2, 128, 256, vocab, 128), small=GPT2Config.gpt2_small(vocab), medium=GPT2Config.gpt2_medium(vocab))[spec.split(":")[1]]
        return cfg, init_hf_style_state_dict(cfg, seed=0)
    import torch
    loader = C.load_hf_pytorch_gpt2 if os.path.exists(os.path.join(spec, "model.safetensors")) or os.path.exists(os.path.join(spec, "pytorch_model.bin")) \
        else C.load_gpt2_checkpoint
    cfg, sd = loader(spec)
    return cfg, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _engine(cfg, params, kind: str = "bf16"):
    """An inference engine over `params`: kind "bf16" = `GPT2Engine`; "f32" / "bf16x3" = `GPT2EngineF32` in that matmul mode."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gpt2 import GPT2Engine
    sd = {k: (v.detach().cpu() if hasattr(v, "detach") else v) for k, v in params.items()}
    if getattr(cfg, "model_family", "gpt2") == "gptj":      # GPT-J runs on the fp32 engine only (its one matmul mode), whatever `kind` says
        from lmrl_gym_amd.gptj_f32_engine import GPTJEngineF32
        return GPTJEngineF32(cfg, sd, _lib.require_gpu())
    if kind == "bf16":
        return GPT2Engine(cfg, sd, _lib.require_gpu())
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    return GPT2EngineF32(cfg, sd, _lib.require_gpu(), matmul=kind)


def _wordle_env(a):
    from lmrl_gym_amd.envs import wordle as W
    vocab = W.Vocabulary.from_file(a.vocab_file) if os.path.exists(a.vocab_file) else W.Vocabulary.builtin(a.vocab_file)
    return vocab, W.ReformatWordleEnvironment(vocab, require_words_in_vocab=True, bad_word_reward=getattr(a, "bad_word_reward", -1.0))


def _device_rollouts(engine, vocab, tok, bsize, bad_word_reward, max_new_tokens):
    """Wordle rollouts with env + policy + loop on the device (`WordleRolloutEngine`); needs single-token letters/symbols, i.e. the
    GPT-2 tokenizer or the Wordle adapter."""
    from lmrl_gym_amd.rollout import WordleRolloutEngine, WordleTokenTable
    table = getattr(tok, "table", None) or WordleTokenTable.from_tokenizer(tok)
    return WordleRolloutEngine(engine, vocab, bsize, tokens=table, max_new_tokens=max_new_tokens, bad_word_reward=bad_word_reward)


def _log(tag, obj):
    print(json.dumps({tag: obj}, default=lambda o: float(o) if isinstance(o, (np.floating, np.integer)) else str(o)), flush=True)


# --------------------------------------------------------------------------------------------------------------- commands
def _scripted_policy(a, vocab):
    """--policy mixture | optimal | optimal-mixture (a --mix-prob coin between the two) with --start-word w1,w2 | default | none."""
    from lmrl_gym_amd.envs import wordle_policies as P
    sw = getattr(a, "start_word", "none")
    start = None if sw == "none" else P.StartWordPolicy(None if sw == "default" else sw.split(","))
    mixture, optimal = P.RandomMixturePolicy(a.prob_smart, vocab), P.OptimalPolicy(vocab, start)
    return dict(mixture=mixture, optimal=optimal)[a.policy] if a.policy != "optimal-mixture" else P.MixturePolicy(a.mix_prob, optimal, mixture)


def cmd_gen_data(a):
    from lmrl_gym_amd import datasets as DS
    vocab, _ = _wordle_env(a)
    if a.device_loop:
        items = DS.generate_wordle_dataset_device(vocab, a.n_data, _scripted_policy(a, vocab), seed=a.seed, bsize=a.bsize)
    elif a.policy != "mixture":
        raise SystemExit("gen-data: --policy optimal / optimal-mixture run on the device loop (--device-loop 1)")
    else:
        items = DS.generate_wordle_dataset(vocab, a.n_data, a.prob_smart, seed=a.seed)
    _log("gen_data", dict(items=DS.write_jsonl(a.out, items), path=a.out, policy=a.policy, device_loop=a.device_loop))


def cmd_optimal_perf(a):
    """Mean reward of optimal play (wordle/misc/optimal_perf.py: OptimalPolicy behind a start word, text_env_eval's summary)."""
    import random
    from lmrl_gym_amd.envs import wordle_policies as P
    vocab, _ = _wordle_env(a)
    a.policy, a.prob_smart = "optimal", 0.0
    loop = P.WordleScriptedRollouts(vocab, _scripted_policy(a, vocab), min(a.bsize, a.n))
    rng = random.Random(a.seed)
    recs = []
    for b0 in range(0, a.n, loop.n):
        k = min(loop.n, a.n - b0)
        recs.append(loop.run([rng.randint(0, 2 ** 31 - 1) for _ in range(k)], [rng.randint(0, 2 ** 31 - 1) for _ in range(k)]))
    loop.close()
    rewards = np.concatenate([r.reward.sum(axis=0) for r in recs])
    lengths = np.concatenate([r.n_turns for r in recs])
    _log("optimal_perf", dict(n=int(len(rewards)), reward_mean=float(rewards.mean()), reward_std=float(rewards.std()),
                              length_mean=float(lengths.mean()), solved=float((rewards > -6).mean())))


def cmd_ilql(a):
    import torch
    from lmrl_gym_amd import _lib, datasets as DS, environment as E
    from lmrl_gym_amd.algorithms import ilql
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.policies import GPT2ValuePolicy, heads_to_engine_layout
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, MLPHeadF32
    dev = _lib.require_gpu()
    tok = _tokenizer()
    cfg, sd = _model(a.model, max(len(tok), 50257))
    mm = dict(matmul="bf16" if a.bf16_activations else "f32")                 # the scripts' bf16_activations / gradient_checkpointing flags
    base = GPT2F32(sd, cfg.n_head, device=dev, gradient_checkpointing=a.gradient_checkpointing, **mm, **_pdrop(a))
    # (the reference calls the target network with train=train too: it drops with its own key, ilql/gpt2/interface.py:149-161)
    target_base, pi_beta = GPT2F32(sd, cfg.n_head, device=dev, **mm, **_pdrop(a)), _engine(cfg, sd, a.policy_engine)
    d, V = cfg.d_model, cfg.vocab
    g = torch.Generator().manual_seed(0)
    # MLPHead init of train_ilql_gpt2.py:224-231: layer-2 kernel 0, layer-2 bias -4.4 (Q heads) ; V head likewise
    mk = lambda out: MLPHeadF32({"dense1.kernel": torch.randn(d, d, generator=g) * 0.02, "dense1.bias": torch.zeros(d),
                                 "dense2.kernel": torch.zeros(d, out), "dense2.bias": torch.full((out,), -4.4)}, dev, **mm)
    tr = ilql.GPT2ILQLTrain(base, mk(V), mk(V), mk(1), tok.pad_token_id, dict(gamma=a.gamma, tau=a.tau, cql_weight=a.cql_weight),
                            target_base=target_base, lr=a.lr, weight_decay=a.weight_decay, grad_accum_steps=a.grad_accum_steps,
                            polyak_alpha=a.polyak_alpha, hard_update_every=None if a.hard_update_every is None else int(a.hard_update_every))
    bs = BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, a.max_length)
    vocab, env = _wordle_env(a)
    if a.device_data:
        # --device-data 1: the gen-data policy plays on the device and its records become the blocked dataset where they lie
        # (datasets.wordle_offline_dataset_device): no jsonl file, no host tokenizer; the train steps take the device batches
        from lmrl_gym_amd.rollout import WordleTokenTable
        table = getattr(tok, "table", None) or WordleTokenTable.from_tokenizer(tok)
        train = DS.wordle_offline_dataset_device(vocab, a.n_data, _scripted_policy(a, vocab), tokens=table, kind="ilql", seed=a.data_seed, bsize=a.data_bsize,
                                                 max_length=a.max_length, bad_word_reward=a.bad_word_reward)
        _log("device_data", dict(episodes=len(train), longest=train.longest, width=int(train.input_ids.shape[1]), policy=a.policy))
        batches = lambda epoch: train.batches(np.random.default_rng(epoch), a.train_bsize, truncate=True)
    else:
        if not a.train_data:
            raise SystemExit("ilql: give --train-data FILE, or --device-data 1 to play the data on the device")
        train = DS.ilql_dataset_from_jsonl(a.train_data, tok, bs)
        batches = lambda epoch: DS.dataloader(np.random.default_rng(epoch), train, a.train_bsize, truncate=True)

    def evaluate():
        # --policy-engine f32 / bf16x3: the heads as the trainer holds them, unrounded (GPT2EngineF32.value_head)
        hl = lambda h: heads_to_engine_layout({k: v.detach().cpu() for k, v in h.p.items()}, cfg.vocab_padded, dev, engine=pi_beta)
        if a.device_rollouts:       # ILQL value policy, env and loop on the GPU
            from lmrl_gym_amd.rollout import WordleRolloutEngine, WordleTokenTable
            table = getattr(tok, "table", None) or WordleTokenTable.from_tokenizer(tok)
            ro = WordleRolloutEngine(pi_beta, vocab, a.policy_bsize, tokens=table, max_new_tokens=min(a.policy_max_output_length, 12),
                                     bad_word_reward=a.bad_word_reward, value_engine=_engine(cfg, base.p, a.policy_engine), q1_head=hl(tr.q1), q2_head=hl(tr.q2),
                                     beta=a.beta)
            _, summary = ro.text_env_eval(a.policy_n_rollouts, seed_generator=iter(range(10 ** 9)), temperature=a.policy_temperature or 1.0,
                                          top_k=int(a.policy_top_k or 0))
            ro.close()
            return summary
        pol = GPT2ValuePolicy(pi_beta, _engine(cfg, base.p, a.policy_engine), hl(tr.q1), hl(tr.q2), a.beta, tok, max_input_length=a.policy_max_input_length,
                              max_new_tokens=a.policy_max_output_length, do_sample=a.policy_do_sample, temperature=a.policy_temperature,
                              top_k=None if a.policy_top_k is None else int(a.policy_top_k), top_p=a.policy_top_p, num_beams=a.policy_num_beams, eos_token_id=tok.encode("\n")[0],
                              out_str_process=lambda x: x.removesuffix("\n") + "\n")
        _, summary = E.text_env_eval(env, pol, n_rollouts=a.policy_n_rollouts, bsize=a.policy_bsize, seed_generator=iter(range(10 ** 9)), verbose=False)
        return summary

    step, keys = 0, _step_keys(a)
    for epoch in range(a.epochs):
        for batch in batches(epoch):
            if a.device_data:
                _, loss, logs = tr.step(**batch, prng_key=keys.next())
            else:
                _, loss, logs = tr.step(batch["input_ids"], batch["should_take_action"], batch["rewards"], batch["dones"],
                                        next_token_ids=batch["next_token_ids"], next_dones=batch["next_dones"], prng_key=keys.next())
            step += 1
            if step % a.log_every == 0 or step == 1:
                _log("train", dict(step=step, epoch=epoch, loss=loss, losses=logs["losses"]))
            if a.max_steps is not None and step >= int(a.max_steps):
                break
        if a.max_steps is not None and step >= int(a.max_steps):
            break
    _log("eval", evaluate())
    if a.out:
        from lmrl_gym_amd import checkpoints as C
        C.save_gpt2_checkpoint(os.path.join(a.out, "base"), cfg, base.p)
        for name, h in (("q1_head", tr.q1), ("q2_head", tr.q2), ("v_head", tr.v)):
            C.save_head_checkpoint(os.path.join(a.out, name), h.p)


def cmd_ppo(a):
    import torch
    from lmrl_gym_amd import _lib, datasets as DS, environment as E
    from lmrl_gym_amd.algorithms import ppo
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ppo_inference import (GPT2PPOInference, text_trajectory_chains_from_interactions, text_trajectory_chains_from_transitions,
                                                       text_trajectory_chains_partially_observed)
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, LinearHeadF32
    dev = _lib.require_gpu()
    tok = _tokenizer(wordle=a.env == "wordle")       # FEN / SAN text needs every byte: the byte tokenizer when no GPT-2 files are around
    cfg, sd = _model(a.model, max(len(tok), 50257))
    mm = dict(matmul="bf16" if a.bf16_activations else "f32")
    pol_f32 = GPT2F32(sd, cfg.n_head, device=dev, gradient_checkpointing=a.gradient_checkpointing, **mm, **_pdrop(a))
    keys = _step_keys(a)
    init_f32 = GPT2F32(sd, cfg.n_head, device=dev, **mm)
    head = LinearHeadF32(dict(kernel=torch.zeros(cfg.d_model, 1), bias=torch.tensor([-4.1])), dev)       # train_ppo_gpt2.py:254-260
    kw = dict(cliprange_value=a.cliprange_value, cliprange=a.cliprange, value_loss_coef=a.value_loss_coef)
    max_len = a.max_input_length + a.max_output_length
    policy = GPT2PPOPolicy(_engine(cfg, sd), tok, max_input_length=a.max_input_length, max_new_tokens=a.max_output_length, do_sample=a.policy_do_sample,
                           temperature=a.policy_temperature, top_k=None if a.policy_top_k is None else int(a.policy_top_k), top_p=a.policy_top_p, num_beams=a.policy_num_beams,
                           eos_token_id=tok.encode("\n")[0], out_str_process=lambda x: x.removesuffix("\n") + "\n")
    inf = GPT2PPOInference(pol_f32, head, tok.pad_token_id, initial_policy=init_f32, tokenizer=tok, loss_kwargs=kw, bc_loss_weight=a.bc_loss_weight)
    tr = ppo.GPT2PPOTrain(pol_f32, head, tok.pad_token_id, kw, lr=a.lr, weight_decay=a.weight_decay, grad_accum_steps=int(a.grad_accum_steps or 1),
                          bc_loss_weight=a.bc_loss_weight)
    ctl = ppo.AdaptiveKLController(a.init_kl_coef, a.kl_target, int(a.kl_horizon)) if a.kl_target is not None and a.kl_horizon is not None \
        else ppo.FixedKLController(a.init_kl_coef)
    bs = BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, max_len)
    bc = DS.MaskDataset.from_jsonl(a.bc_data, tok, bs) if a.bc_data else None
    if a.env == "chess":        # configs[3]: online PPO against the chess env (chess/ppo/train_ppo_gpt2_online.py:201-222)
        from lmrl_gym_amd.envs import chess as C
        start = C.large_piece_random_endgame(a.chess_pieces) if a.chess_pieces else None
        env = C.FenChessHistoryEnv(max_moves=a.chess_max_moves, from_position=start, random_opponent=bool(a.chess_random_opponent),
                                   **({} if a.chess_random_opponent else dict(engine_path=a.chess_engine, engine_options={"Use NNUE": a.chess_use_nnue},
                                                                              movetime_ms=a.chess_movetime_ms)))
        vocab = None
    elif a.env == "maze":       # configs[0]'s online script: llm_rl_scripts/maze/ppo/train_ppo_online.py:260-300, 431-483
        from lmrl_gym_amd.envs import maze as M
        env = M.setup_maze_env(a.maze_name, a.maze_describe_function, a.maze_reward_function, last_k=a.maze_last_k, max_steps=a.maze_max_steps)
        vocab = None
    elif a.env == "twenty-questions":       # twenty_questions/ppo/train_ppo.py: a second resident model answers the questions inside the loop
        from lmrl_gym_amd.envs import twenty_questions as TQ
        ocfg, osd = _model(a.tq_oracle_model or a.model, max(len(tok), 50257))
        tq_oracle = _engine(ocfg, osd)
        words = TQ.get_default_word_list()[: a.tq_words]
        env = TQ.BatchedTwentyQuestionsPolicyEnvironment(TQ.GPT2EngineOracle(tq_oracle, tok, max_input_length=a.tq_oracle_max_input_length, max_new_tokens=4,
                                                                             eos_token_id=tok.encode("\n")[0]), words, a.tq_max_conversation_length, a.rollout_bsize)
        vocab = None
    else:
        vocab, env = _wordle_env(a)
    step = 0
    limit = None if a.max_steps is None else int(a.max_steps)
    # --device-rollouts: the whole iteration stays in HBM — rollout records -> PPO data -> device batches -> train steps -> the trainer's
    # parameters copied into the engine in place (WordleRolloutEngine.ppo_rollouts, algorithms/ppo_device.py); --resident 0: the host-array path
    resident = bool(a.device_rollouts) and bool(a.resident)

    def chess_rollouts():
        # env + policy + lock-step loop on the GPU (ChessRolloutEngine): the device opponent for --chess-random-opponent 1, else the env's engine pool
        from lmrl_gym_amd.chess_rollout import ChessRolloutEngine
        return ChessRolloutEngine(policy.engine, tok, env, a.rollout_bsize, max_new_tokens=min(a.max_output_length, 12), eos_token_id=tok.encode("\n")[0],
                                  max_input_length=a.max_input_length, opponent="device" if a.chess_random_opponent else env._vec.engine)

    def tq_rollouts():
        # both models, the env's text rules and the lock-step loop on the GPU (TwentyQuestionsRolloutEngine)
        from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
        return TwentyQuestionsRolloutEngine(policy.engine, tq_oracle, tok, env, a.rollout_bsize, max_new_tokens=min(a.max_output_length, 12),
                                            eos_token_id=tok.encode("\n")[0], max_input_length=a.max_input_length,
                                            oracle_max_input_length=a.tq_oracle_max_input_length)
    if resident and a.env == "chess":
        ro_res = chess_rollouts()
    elif resident and a.env == "twenty-questions":
        ro_res = tq_rollouts()
    elif resident and a.env == "maze":
        from lmrl_gym_amd.maze_rollout import MazeRolloutEngine
        ro_res = MazeRolloutEngine(policy.engine, tok, env, a.rollout_bsize, max_new_tokens=min(a.max_output_length, 12), eos_token_id=tok.encode("\n")[0],
                                   max_input_length=a.max_input_length)
    else:
        ro_res = _device_rollouts(policy.engine, vocab, tok, a.rollout_bsize, a.bad_word_reward, min(a.max_output_length, 12)) if resident else None
    for rnd in range(a.n_rounds):
        if limit is not None and step >= limit:
            break
        if resident:
            warp = dict(top_k=int(a.policy_top_k or 0)) if a.env in ("maze", "chess") else dict(top_k=int(a.policy_top_k or 0), top_p=float(a.policy_top_p or 0.0))
            ds, kls, summary = ro_res.ppo_rollouts(inf, a.n_rollouts, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)), gamma=a.gamma, lam=a.lam,
                                                   kl_weight=ctl.value, max_length=max_len, use_advantage_whitening=a.use_advantage_whitening,
                                                   temperature=a.policy_temperature or 1.0, sample_seed=rnd, bsize=max(a.ppo_data_bsize, 64), **warp)
            mean_kl = float(kls.cpu().numpy().mean()) if kls.numel() else 0.0
            ctl.update(mean_kl, a.train_bsize)
            _log("data_collection", dict(round=rnd, env_interaction=summary, mean_kl=mean_kl, kl_ctrl_value=ctl.value, n_chains=len(ds), device_resident=True))
            bc_iter = None
            for epoch in range(a.epochs):
                if limit is not None and step >= limit:
                    break
                for batch in ds.batches(np.random.default_rng(rnd * 1000 + epoch), min(a.train_bsize, len(ds)), truncate=True,
                                        width=ds.trimmed_width() if a.trim_batches else None):
                    extra = {}
                    if bc is not None:
                        if bc_iter is None:
                            bc_iter = DS.dataloader(np.random.default_rng(7 + step), bc, int(a.train_bc_bsize or a.train_bsize), truncate=True)
                        try:
                            bb = next(bc_iter)
                        except StopIteration:
                            bc_iter = DS.dataloader(np.random.default_rng(7 + step), bc, int(a.train_bc_bsize or a.train_bsize), truncate=True)
                            bb = next(bc_iter)
                        extra = dict(bc_data_input_ids=bb["input_ids"], bc_data_input_training_mask=bb["input_training_mask"])
                    _, loss, logs = tr.step(**batch, **extra, prng_key=keys.next())
                    step += 1
                    _log("train", dict(step=step, round=rnd, loss=loss))
                    if limit is not None and step >= limit:
                        break
            ro_res.load_params(pol_f32.p)
            continue
        if a.device_rollouts and a.env == "maze":
            from lmrl_gym_amd.maze_rollout import MazeRolloutEngine
            ro = MazeRolloutEngine(policy.engine, tok, env, a.rollout_bsize, max_new_tokens=min(a.max_output_length, 12), eos_token_id=tok.encode("\n")[0],
                                   max_input_length=a.max_input_length)
            raw, summary = ro.text_env_eval(a.n_rollouts, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)), temperature=a.policy_temperature or 1.0,
                                            top_k=int(a.policy_top_k or 0), sample_seed=rnd)
            ro.close()
        elif a.device_rollouts and a.env == "chess":
            ro = chess_rollouts()
            raw, summary = ro.text_env_eval(a.n_rollouts, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)), temperature=a.policy_temperature or 1.0,
                                            top_k=int(a.policy_top_k or 0), sample_seed=rnd)
            ro.close()
        elif a.device_rollouts and a.env == "twenty-questions":
            ro = tq_rollouts()
            raw, summary = ro.text_env_eval(a.n_rollouts, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)), temperature=a.policy_temperature or 1.0,
                                            top_k=int(a.policy_top_k or 0), top_p=float(a.policy_top_p or 0.0), sample_seed=rnd)
            ro.close()
        elif a.device_rollouts:     # env + policy + lock-step loop on the GPU; same (interactions, summary) as text_env_eval
            ro = _device_rollouts(policy.engine, vocab, tok, a.rollout_bsize, a.bad_word_reward, min(a.max_output_length, 12))
            raw, summary = ro.text_env_eval(a.n_rollouts, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)), temperature=a.policy_temperature or 1.0,
                                            top_k=int(a.policy_top_k or 0), top_p=float(a.policy_top_p or 0.0), sample_seed=rnd, concurrent=a.rollout_lanes)
            ro.close()
        else:
            raw, summary = E.text_env_eval(env, policy, n_rollouts=a.n_rollouts, bsize=a.rollout_bsize, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)),
                                           verbose=False)
        if a.env == "maze" and a.maze_last_k != 1:      # item windows: the partially observed script's joined-state chains (partially_observed_ppo_online.py:372-398)
            chains = text_trajectory_chains_partially_observed(raw)
        else:
            chains = text_trajectory_chains_from_transitions(raw) if a.env in ("chess", "maze") else text_trajectory_chains_from_interactions(raw, tok, max_len, a.gamma)
        datas, kls = inf.get_ppo_data_from_text_trajectory_chain(chains, bsize=a.ppo_data_bsize, max_length=max_len, gamma=a.gamma, lam=a.lam,
                                                                 kl_weight=ctl.value, use_advantage_whitening=a.use_advantage_whitening)
        mean_kl = float(kls.mean()) if len(kls) else 0.0
        ctl.update(mean_kl, a.train_bsize)
        _log("data_collection", dict(round=rnd, env_interaction=summary, mean_kl=mean_kl, kl_ctrl_value=ctl.value, n_chains=len(chains)))
        ds = ppo.PPODataset.from_ppo_data_list(datas, tok, bs)
        bc_iter = None
        for epoch in range(a.epochs):
            if limit is not None and step >= limit:
                break
            for batch in DS.dataloader(np.random.default_rng(rnd * 1000 + epoch), ds, min(a.train_bsize, len(ds)), truncate=True):
                extra = {}
                if bc is not None:
                    if bc_iter is None:
                        bc_iter = DS.dataloader(np.random.default_rng(7 + step), bc, int(a.train_bc_bsize or a.train_bsize), truncate=True)
                    try:
                        bb = next(bc_iter)
                    except StopIteration:
                        bc_iter = DS.dataloader(np.random.default_rng(7 + step), bc, int(a.train_bc_bsize or a.train_bsize), truncate=True)
                        bb = next(bc_iter)
                    extra = dict(bc_data_input_ids=bb["input_ids"], bc_data_input_training_mask=bb["input_training_mask"])
                _, loss, logs = tr.step(**batch, **extra, prng_key=keys.next())
                step += 1
                _log("train", dict(step=step, round=rnd, loss=loss))
                if a.max_steps is not None and step >= int(a.max_steps):
                    break
        policy.set_params(_engine(cfg, pol_f32.p))
    _, summary = E.text_env_eval(env, policy, n_rollouts=a.n_rollouts, bsize=a.rollout_bsize, seed_generator=iter(range(10 ** 8, 10 ** 9)), verbose=False)
    _log("eval", summary)


def cmd_filtered_bc(a):
    """Online filtered BC (LLM_RL/algorithms/online_filtered_bc/train.py + wordle/online_filtered_bc/train_online_filtered_bc_gpt2.py:198-278):
    every round: rollouts with the current policy, keep the top `filter_percengage` episodes by total reward, BC on their action tokens."""
    import torch
    from lmrl_gym_amd import _lib, datasets as DS, environment as E
    from lmrl_gym_amd.algorithms import bc
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32
    dev = _lib.require_gpu()
    tok = _tokenizer()
    cfg, sd = _model(a.model, max(len(tok), 50257))
    model = GPT2F32(sd, cfg.n_head, device=dev, matmul="bf16" if a.bf16_activations else "f32", gradient_checkpointing=a.gradient_checkpointing, **_pdrop(a))
    keys = _step_keys(a)
    tr = bc.GPT2BCTrain(model, tok.pad_token_id, lr=a.lr, weight_decay=a.weight_decay, grad_accum_steps=int(a.grad_accum_steps or 1))
    policy = GPT2PPOPolicy(_engine(cfg, sd), tok, max_input_length=a.max_input_length, max_new_tokens=a.max_output_length, do_sample=a.policy_do_sample,
                           temperature=a.policy_temperature, top_k=None if a.policy_top_k is None else int(a.policy_top_k), top_p=a.policy_top_p, num_beams=a.policy_num_beams,
                           eos_token_id=tok.encode("\n")[0], out_str_process=lambda x: x.removesuffix("\n") + "\n")
    vocab, env = _wordle_env(a)
    bs = BlockingStrategy(Padding.RIGHT, Truncation.LEFT, a.max_input_length + a.max_output_length)
    step = 0
    limit = None if a.max_steps is None else int(a.max_steps)
    if a.device_data:
        # --device-data 1: the round never leaves the device — records -> filter_records (one [n] score readback) -> DeviceMaskDataset -> steps on
        # device batches -> the trainer's parameters into the SAME engine in place (captured episodes stay valid)
        if not a.device_rollouts:
            raise SystemExit("filtered-bc --device-data 1 needs --device-rollouts 1")
        from lmrl_gym_amd.algorithms import offline_device as OD
        ro = _device_rollouts(policy.engine, vocab, tok, a.rollout_bsize, a.bad_word_reward, min(a.max_output_length, 12))
        for rnd in range(a.n_rounds):
            if limit is not None and step >= limit:
                break
            rec, summary = ro.record_rollouts(a.n_rollouts, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)), temperature=a.policy_temperature or 1.0,
                                              top_k=int(a.policy_top_k or 0), top_p=float(a.policy_top_p or 0.0), sample_seed=rnd)
            keep = OD.filter_records(rec, top_fraction=a.filter_percengage)
            kept = [int(i) for i in keep.rows_host]
            scores = OD.record_returns(rec).cpu().numpy()
            _log("data_collection", dict(round=rnd, env_interaction=summary, kept=len(kept), kept_episodes=kept,
                                         reward_cutoff=min((float(scores[i]) for i in kept), default=None), device_resident=True))
            if not kept:
                continue
            ds = OD.mask_data_from_records(rec, bs, tok.pad_token_id, keep=keep)
            for epoch in range(a.epochs):
                if limit is not None and step >= limit:
                    break
                for batch in ds.batches(np.random.default_rng(rnd * 1000 + epoch), min(a.train_bsize, len(ds)), truncate=True):
                    _, loss, _ = tr.step(**batch, prng_key=keys.next())
                    step += 1
                    _log("train", dict(step=step, round=rnd, loss=loss))
                    if limit is not None and step >= limit:
                        break
            ro.load_params(model.p)
        _, summary = ro.record_rollouts(a.n_rollouts, seed_generator=iter(range(10 ** 8, 10 ** 9)), temperature=a.policy_temperature or 1.0,
                                        top_k=int(a.policy_top_k or 0), top_p=float(a.policy_top_p or 0.0), sample_seed=a.n_rounds)
        ro.close()
        _log("eval", summary)
        return
    for rnd in range(a.n_rounds):
        if limit is not None and step >= limit:      # the step budget ends the run: no further rollouts, epochs or rounds
            break
        if a.device_rollouts:
            ro = _device_rollouts(policy.engine, vocab, tok, a.rollout_bsize, a.bad_word_reward, min(a.max_output_length, 12))
            raw, summary = ro.text_env_eval(a.n_rollouts, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)), temperature=a.policy_temperature or 1.0,
                                            top_k=int(a.policy_top_k or 0), top_p=float(a.policy_top_p or 0.0), sample_seed=rnd, concurrent=a.rollout_lanes)
            ro.close()
        else:
            raw, summary = E.text_env_eval(env, policy, n_rollouts=a.n_rollouts, bsize=a.rollout_bsize, seed_generator=iter(range(rnd * 10 ** 6, 10 ** 9)),
                                           verbose=False)
        segs = [[(t.text, float(t.is_action)) for t in ep[-1].post_transition_history] for ep in raw]
        rewards = [sum(t.reward for t in ep) for ep in raw]
        top = sorted(range(len(segs)), key=lambda i: rewards[i], reverse=True)[: int(len(segs) * a.filter_percengage)]
        _log("data_collection", dict(round=rnd, env_interaction=summary, kept=len(top), kept_episodes=list(top),
                                     reward_cutoff=min((rewards[i] for i in top), default=None)))
        if not top:
            continue
        ds = DS.MaskDataset.blocked_from_str_segments([segs[i] for i in top], tok, bs)
        for epoch in range(a.epochs):
            if limit is not None and step >= limit:
                break
            for batch in DS.dataloader(np.random.default_rng(rnd * 1000 + epoch), ds, min(a.train_bsize, len(ds)), truncate=True):
                _, loss, _ = tr.step(batch["input_ids"], batch["input_training_mask"] > 0, prng_key=keys.next())
                step += 1
                _log("train", dict(step=step, round=rnd, loss=loss))
                if limit is not None and step >= limit:
                    break
        policy.set_params(_engine(cfg, model.p))
    _, summary = E.text_env_eval(env, policy, n_rollouts=a.n_rollouts, bsize=a.rollout_bsize, seed_generator=iter(range(10 ** 8, 10 ** 9)), verbose=False)
    _log("eval", summary)


def cmd_bc_eval(a):
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    tok = _tokenizer()
    cfg, sd = _model(a.model, max(len(tok), 50257), a.model_family)
    policy = GPT2PPOPolicy(_engine(cfg, sd), tok, max_input_length=a.policy_max_input_length, max_new_tokens=a.policy_max_output_length,
                           do_sample=a.policy_do_sample, temperature=a.policy_temperature, top_k=None if a.policy_top_k is None else int(a.policy_top_k),
                           top_p=a.policy_top_p, num_beams=a.policy_num_beams, eos_token_id=tok.encode("\n")[0], out_str_process=lambda x: x.removesuffix("\n") + "\n")
    vocab, env = _wordle_env(a)
    if a.device_rollouts:       # same call, env + policy + loop on the GPU
        ro = _device_rollouts(policy.engine, vocab, tok, a.policy_bsize, -1.0, min(a.policy_max_output_length, 12))
        _, summary = ro.text_env_eval(a.policy_n_rollouts, seed_generator=iter(range(10 ** 9)), temperature=a.policy_temperature or 1.0,
                                      top_k=int(a.policy_top_k or 0), concurrent=a.rollout_lanes)
        ro.close()
    else:
        _, summary = E.text_env_eval(env, policy, n_rollouts=a.policy_n_rollouts, bsize=a.policy_bsize, seed_generator=iter(range(10 ** 9)), verbose=False)
    _log("eval", summary)


def cmd_maze_eval(a):
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.envs import maze as M
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    tok = _tokenizer(wordle=False)
    cfg, sd = _model(a.model, max(len(tok), 50257), a.model_family)
    policy = GPT2PPOPolicy(_engine(cfg, sd, a.policy_engine), tok, max_input_length=a.max_input_length, max_new_tokens=a.max_output_length, do_sample=False,
                           eos_token_id=tok.encode("\n")[0], out_str_process=lambda x: x.removesuffix("\n") + "\n")
    env = M.setup_maze_env(a.maze_name, a.describe_function, a.reward_function, last_k=a.last_k, max_steps=a.max_steps)
    starts = [tuple(p) for p in np.argwhere(M.double_t_maze() == 0).tolist()]        # one rollout per free cell (fully_observed_bc.py:262-283)
    results = []
    for i in range(0, len(starts), a.generation_bsize):
        opts = [dict(init_position=p) for p in starts[i:i + a.generation_bsize]]
        inter = E.interact_environment(env, policy, env_seed=[None] * len(opts), env_options=opts, bsize=len(opts))
        results += [dict(start=starts[i + k], reward=sum(t.reward for t in ep), steps=len(ep), done=ep[-1].done) for k, ep in enumerate(inter)]
    _log("maze_eval", dict(avg_reward=float(np.mean([r["reward"] for r in results])), avg_steps=float(np.mean([r["steps"] for r in results])),
                           n=len(results), move_accuracy=M.compute_move_accuracy(policy)))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name, fn, defaults in (("ilql", cmd_ilql, ILQL_DEFAULTS), ("ppo", cmd_ppo, PPO_DEFAULTS), ("filtered-bc", cmd_filtered_bc, FILTERED_BC_DEFAULTS),
                               ("bc-eval", cmd_bc_eval, BC_EVAL_DEFAULTS),
                               ("maze-eval", cmd_maze_eval, MAZE_EVAL_DEFAULTS)):
        p = sub.add_parser(name)
        p.set_defaults(fn=fn)
        p.add_argument("--model", default="random:tiny", help="checkpoint directory (reference layout or HF PyTorch) or random:<tiny|small>")
        p.add_argument("--model-family", default="gpt2", choices=["gpt2", "gptj"],
                       help="gptj (bc-eval and maze-eval only, without --device-rollouts): --model is random:gptj-tiny or a GPT-J checkpoint directory; "
                            "the policy runs on GPTJEngineF32 (fp32)")
        p.add_argument("--vocab-file", default="wordle_official_400.txt")
        p.add_argument("--out", default=None)
        p.add_argument("--device-rollouts", type=int, default=0, help="1 = run the rollouts (bc-eval, ilql evaluation, ppo data collection: Wordle, Maze, chess) on the device-resident engine")
        p.add_argument("--rollout-lanes", type=int, default=1, help="device rollouts: independent episode batches in flight at once "
                                                                     "(WordleRolloutEngine.text_env_eval(concurrent=n); >= 4 batches use the graph path)")
        _add(p, defaults)
    for name in ("ilql", "filtered-bc", "ppo"):
        p = sub.choices[name]
        for site in ("resid", "attn", "embd"):
            p.add_argument(f"--{site}-pdrop", type=float, default=0.0,
                           help=f"GPT-2 {site}_pdrop of the train model (default 0.0 = no dropout).  The reference's values: BC 0.05 on all three "
                                "(train_bc_gpt2.py), ILQL and MC 0.1 on all three (the HF GPT2Config default, which its scripts leave alone), PPO and online "
                                "filtered BC 0.0")
        p.add_argument("--seed", type=int, default=0, help="seed of the dropout key (jax_prng.prng_key(seed), split once per train step)")
    sub.choices["ilql"].add_argument("--train-data", default=None)
    for name in ("ilql", "filtered-bc"):
        sub.choices[name].add_argument("--device-data", type=int, default=0,
                                       help="1 = datasets are built on the device from rollout records and the train steps take device batches: ilql plays "
                                            "--n-data episodes of the gen-data --policy instead of reading --train-data; filtered-bc (with --device-rollouts 1) "
                                            "keeps every round in HBM and loads the new weights into the engine in place")
    il = sub.choices["ilql"]
    il.add_argument("--n-data", type=int, default=1000); il.add_argument("--prob-smart", type=float, default=0.5)
    il.add_argument("--policy", default="mixture", choices=["mixture", "optimal", "optimal-mixture"]); il.add_argument("--mix-prob", type=float, default=0.5)
    il.add_argument("--start-word", default="none"); il.add_argument("--data-seed", type=int, default=0); il.add_argument("--data-bsize", type=int, default=1024)
    sub.choices["ilql"].add_argument("--eval-data", default=None)
    sub.choices["ilql"].add_argument("--policy-engine", default="bf16", choices=["bf16", "f32", "bf16x3"],
                                     help="evaluation engines of pi_beta and the value base: bf16 GPT2Engine (default) or GPT2EngineF32 in that matmul mode "
                                          "(the reference evaluates in float32 by default) with unrounded heads")
    sub.choices["maze-eval"].add_argument("--policy-engine", default="bf16", choices=["bf16", "f32", "bf16x3"],
                                          help="evaluation engine of the policy: bf16 GPT2Engine (default) or GPT2EngineF32 in that matmul mode "
                                               "(the reference's Maze scripts evaluate in float32 by default)")
    sub.choices["ppo"].add_argument("--bc-data", default=None)
    pp = sub.choices["ppo"]
    pp.add_argument("--env", default="wordle", choices=["wordle", "chess", "maze", "twenty-questions"])
    pp.add_argument("--tq-max-conversation-length", type=int, default=20); pp.add_argument("--tq-oracle-model", default=None, help="default: --model")
    pp.add_argument("--tq-oracle-max-input-length", type=int, default=256); pp.add_argument("--tq-words", type=int, default=None, help="only the first N objects")
    pp.add_argument("--maze-name", default="double_t_maze"); pp.add_argument("--maze-describe-function", default="describe_observation_give_position")
    pp.add_argument("--maze-reward-function", default="standard_reward"); pp.add_argument("--maze-last-k", type=int, default=1)
    pp.add_argument("--maze-max-steps", type=int, default=100)
    pp.add_argument("--resident", type=int, default=1, help="with --device-rollouts 1: 1 (default) = the device-resident iteration, 0 = device rollouts feeding the host-array PPO data path")
    pp.add_argument("--trim-batches", type=int, default=1, help="device-resident loop: train on batches cut to the round's longest episode (multiple of 64) instead of "
                                                                  "max_input_length + max_output_length columns — same loss and gradients, fewer padded rows")
    pp.add_argument("--chess-engine", default=os.environ.get("CHESS_ENGINE_PATH"), help="UCI engine binary (the reference: stockfish/stockfish-ubuntu-20.04-x86-64-avx2)")
    pp.add_argument("--chess-use-nnue", default="true", help="'false' for a binary built without the net file")
    pp.add_argument("--chess-random-opponent", type=int, default=0)
    pp.add_argument("--chess-pieces", default=None, help="e.g. kQK: start every round from a random endgame of this material (large_piece_random_endgame)")
    pp.add_argument("--chess-max-moves", type=int, default=400)
    pp.add_argument("--chess-movetime-ms", type=int, default=100)
    g = sub.add_parser("gen-data")
    g.set_defaults(fn=cmd_gen_data)
    g.add_argument("--n-data", type=int, default=1000); g.add_argument("--prob-smart", type=float, default=0.5)
    g.add_argument("--seed", type=int, default=0); g.add_argument("--out", required=True); g.add_argument("--vocab-file", default="wordle_official_400.txt")
    o = sub.add_parser("optimal-perf")
    o.set_defaults(fn=cmd_optimal_perf)
    o.add_argument("--n", type=int, default=1000); o.add_argument("--seed", type=int, default=0); o.add_argument("--vocab-file", default="wordle_official_400.txt")
    g.add_argument("--policy", default="mixture", choices=["mixture", "optimal", "optimal-mixture"])
    g.add_argument("--mix-prob", type=float, default=0.5, help="optimal-mixture: probability of the optimal policy per turn")
    g.add_argument("--device-loop", type=int, default=0, help="1 = policy, env and episode loop on the device (generate_wordle_dataset_device)")
    for p in (g, o):
        p.add_argument("--start-word", default="raise" if p is o else "none", help="first-turn words of OptimalPolicy: w1,w2,... | default | none")
        p.add_argument("--bsize", type=int, default=1024)
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if getattr(a, "model_family", "gpt2") == "gptj":
        # GPT-J is inference on the fp32 engine through the text policies: no train step, no device-resident rollout loop
        if a.cmd not in ("bc-eval", "maze-eval"):
            raise SystemExit(f"--model-family gptj is not available for `{a.cmd}`: GPT-J training is not implemented (bc-eval and maze-eval take it)")
        if getattr(a, "device_rollouts", 0):
            raise SystemExit("--model-family gptj is not available with --device-rollouts 1 (the device-resident rollout loops run GPT-2 engines only); "
                             "use --device-rollouts 0")
        if getattr(a, "policy_num_beams", 1) > 1:
            raise SystemExit("--model-family gptj is not available with --policy-num-beams > 1 (beam search runs on GPT-2 engines only)")
    if getattr(a, "policy_num_beams", 1) > 1 and getattr(a, "device_rollouts", 0):
        # the device-resident rollout engines sample (temperature / top_k / top_p); beam search runs in the text policies' act() only
        raise SystemExit("--policy-num-beams > 1 is not available with --device-rollouts 1 (the device rollout loops do not run beam search); "
                         "use --device-rollouts 0")
    a.fn(a)


if __name__ == "__main__":
    main()
