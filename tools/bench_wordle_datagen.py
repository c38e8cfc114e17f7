"""Offline Wordle data generation: episodes/s and env-steps/s of
  (a) `datasets.generate_wordle_dataset` — env on the device, words chosen on the host per turn,
  (b) `WordleScriptedRollouts` with the same RandomMixturePolicy — policy, env and loop on the device,
  (c) `WordleScriptedRollouts` with OptimalPolicy behind a start word (no counterpart in (a)).
One JSON line per run.

    python tools/bench_wordle_datagen.py [--episodes 16384] [--vocab wordle_official_400.txt] [--prob-smart 0.5] [--bsize 16384]
                                         [--legs a,b,c] [--host-episodes 2048] [--graph 1] [--reps 7]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _loop_leg(vocab, policy, episodes, bsize, graph, reps):
    import torch
    from lmrl_gym_amd.envs import wordle_policies as P
    loop = P.WordleScriptedRollouts(vocab, policy, min(bsize, episodes))
    n_batches = -(-episodes // loop.n)
    seeds = lambda b: (torch.arange(b * loop.n, (b + 1) * loop.n, dtype=torch.int64, device=loop.dev),           # noqa: E731
                       torch.arange(b * loop.n, (b + 1) * loop.n, dtype=torch.int64, device=loop.dev) + (1 << 20))
    loop.run_device(*seeds(10 ** 6), use_graph=graph)      # warm: MT table, first-turn scores, graph capture
    torch.cuda.synchronize()
    times = []
    for rep in range(reps):                                  # median of `reps` passes over fresh seeds
        t0 = time.perf_counter()
        steps = 0
        for b in range(n_batches):
            loop.run_device(*seeds(rep * n_batches + b), use_graph=graph)
            steps += int(loop.n_turns.sum().item())         # one sync per batch of episodes: what a consumer of the records pays
        times.append(time.perf_counter() - t0)
    dt = sorted(times)[len(times) // 2]
    reward = float(loop.reward.sum(dim=0).mean().item())
    loop.close()
    n = n_batches * loop.n
    return dict(episodes=n, reps=reps, seconds=dt, episodes_per_s=n / dt, env_steps_per_s=steps / dt, mean_reward_last_batch=reward)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=16384)
    ap.add_argument("--host-episodes", type=int, default=2048, help="episodes of leg (a): the host generator is measured on fewer and reported per second")
    ap.add_argument("--vocab", default="wordle_official_400.txt")
    ap.add_argument("--prob-smart", type=float, default=0.5)
    ap.add_argument("--bsize", type=int, default=16384)
    ap.add_argument("--start-word", default="raise")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from lmrl_gym_amd import datasets as DS
    from lmrl_gym_amd.envs import wordle as W, wordle_policies as P
    vocab = W.Vocabulary.builtin(a.vocab)
    out = dict(bench="wordle_datagen", vocab=a.vocab, n_words=vocab.all_vocab_size(), prob_smart=a.prob_smart, bsize=a.bsize)
    legs = a.legs.split(",")
    if "a" in legs:
        DS.generate_wordle_dataset(vocab, 64, a.prob_smart, seed=1, bsize=64)
        t0 = time.perf_counter()
        items = DS.generate_wordle_dataset(vocab, a.host_episodes, a.prob_smart, seed=0, bsize=min(a.bsize, 1024))
        dt = time.perf_counter() - t0
        steps = sum((len(it["sequence"]) - 1) // 2 for it in items)
        out["a_host_policy"] = dict(episodes=len(items), seconds=dt, episodes_per_s=len(items) / dt, env_steps_per_s=steps / dt)
    if "b" in legs:
        out["b_device_mixture"] = _loop_leg(vocab, P.RandomMixturePolicy(a.prob_smart, vocab), a.episodes, a.bsize, bool(a.graph), a.reps)
    if "c" in legs:
        start = None if a.start_word == "none" else P.StartWordPolicy(a.start_word.split(","))
        out["c_device_optimal"] = _loop_leg(vocab, P.OptimalPolicy(vocab, start), a.episodes, a.bsize, bool(a.graph), a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
