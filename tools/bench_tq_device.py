"""Throughput of the device-resident Twenty Questions rollout loop against the generic text path on the same engines, seeds and box.

    python tools/bench_tq_device.py [--envs 1024] [--guesser medium] [--oracle large] [--max-conversation-length 20] [--max-new 12] [--runs 3]

Random weights, the byte tokenizer, the default object list, sampling at temperature 1.  Two legs, one JSON line:

  device   `TwentyQuestionsRolloutEngine` under graph replay: both models, the text rules and the loop in HBM
  host     `E.interact_environment(BatchedTwentyQuestionsPolicyEnvironment(GPT2EngineOracle), GPT2PPOPolicy)`: today's path (question text up, B oracle
           prompt strings, tokenizer, the oracle policy, regex, `is_done`, history text down)

An env-step is one question of one live game; each leg reports env-steps/s over `--runs` timed runs after a warm-up (median, and each run).
Both legs end with the episode batch as `List[List[InteractionTransition]]` on the host: the device leg's timed region includes `interactions()`, i.e.
the record's readback, the host's re-judgement of flagged turns and the host lists (`device_loop_only`: the same runs without that tail).
`ratio` = device / host.  The workload: random weights over a 50257-id vocabulary with the byte tokenizer sample mostly ids that decode to nothing, so
most questions are "\n", almost never the canonical encoding of their own text (the guesser re-forwards them from the canonical ids), and the oracle's
answers parse to "No." — the same for both legs, and the models' work per turn does not depend on it.  `--legs device` / `--legs host` runs one leg alone (a profile of one episode; a run split over two time limits).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--guesser", default="medium", choices=["tiny", "small", "medium", "large"])
    ap.add_argument("--oracle", default="large", choices=["tiny", "small", "medium", "large"])
    ap.add_argument("--max-conversation-length", type=int, default=20)
    ap.add_argument("--max-new", type=int, default=12)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="device,host")
    a = ap.parse_args(argv)
    import torch
    import lmrl_gym_amd  # noqa: F401
    from lmrl_gym_amd import _lib, environment as E
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.envs import twenty_questions as TQ
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine, init_hf_style_state_dict
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
    dev = _lib.require_gpu()
    tok = ByteTokenizer()
    nl = tok.encode("\n")[0]
    TQ.set_pos_tagger(TQ.rule_pos_tag)
    mk = dict(tiny=lambda: GPT2Config(2, 2, 128, 256, 50257, 1024), small=lambda: GPT2Config.gpt2_small(50257), medium=lambda: GPT2Config.gpt2_medium(50257),
              large=lambda: GPT2Config.gpt2_large(50257))
    gcfg, ocfg = mk[a.guesser](), mk[a.oracle]()
    guesser = GPT2Engine(gcfg, init_hf_style_state_dict(gcfg, seed=0), dev)
    oracle = GPT2Engine(ocfg, init_hf_style_state_dict(ocfg, seed=1), dev)
    B, T, G = a.envs, a.max_conversation_length, a.max_new
    max_in = -(-(len(TQ.INITIAL_STR) + T * (G + 1 + 5)) // 16) * 16
    omax_in = 256
    words = TQ.get_default_word_list()
    seeds = list(range(1000, 1000 + B))
    out = dict(envs=B, guesser=a.guesser, oracle=a.oracle, max_conversation_length=T, max_new_tokens=G, runs=a.runs, legs=[])

    def timed(fn):
        for _ in range(a.warmup):
            fn()                                    # warm-up (graph capture, allocations)
        torch.cuda.synchronize()
        rates = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            steps = fn()
            torch.cuda.synchronize()
            rates.append(steps / (time.perf_counter() - t0))
        return rates
    legs = a.legs.split(",")
    if "device" in legs:
        env = TQ.BatchedTwentyQuestionsPolicyEnvironment(None, words, T, B)
        ro = TwentyQuestionsRolloutEngine(guesser, oracle, tok, env, B, G, nl, max_in, omax_in)
        episode = [0]

        def device_run(lists=True):
            ro.run_episode(seeds, None, temperature=1.0, sample_seed=3, episode=episode[0], use_graph=True, sync_every=0)
            episode[0] += 1
            if lists:
                return sum(len(ep) for ep in ro.interactions())
            return int(ro.traj["n_turns"].sum().item())
        rates = timed(device_run)
        loop = timed(lambda: device_run(False))
        out["legs"].append(dict(leg="device", env_steps_per_s=float(np.median(rates)), runs=[float(x) for x in rates], judge=ro.judge,
                                device_loop_only=float(np.median(loop)), yes_last_run=int(ro.traj["answer"].sum().item())))
        ro.close()
        del ro
    if "host" in legs:
        env = TQ.BatchedTwentyQuestionsPolicyEnvironment(TQ.GPT2EngineOracle(oracle, tok, max_input_length=omax_in, max_new_tokens=4, eos_token_id=nl), words, T, B)
        pol = GPT2PPOPolicy(guesser, tok, max_input_length=max_in, max_new_tokens=G, do_sample=True, temperature=1.0, eos_token_id=nl,
                            out_str_process=lambda x: x.removesuffix("\n") + "\n")

        def host_run():
            inter = E.interact_environment(env, pol, env_seed=seeds, bsize=B)
            return sum(len(ep) for ep in inter)
        rates = timed(host_run)
        out["legs"].append(dict(leg="host", env_steps_per_s=float(np.median(rates)), runs=[float(x) for x in rates]))
    by = {l["leg"]: l["env_steps_per_s"] for l in out["legs"]}
    if "device" in by and "host" in by:
        out["ratio"] = by["device"] / by["host"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
