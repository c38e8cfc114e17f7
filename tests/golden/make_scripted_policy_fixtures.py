"""Generates tests/golden/wordle_scripted_policies.json by RUNNING the reference's scripted Wordle policies and env
(llm_rl_scripts/wordle/env/{scripted_policies,env,game}.py, LLM_RL/environment.py) — nothing of the reference is stored but
its results.

    python tests/golden/make_scripted_policy_fixtures.py

Determinism contract of the fixtures: episode i runs `random.seed(policy_seed_i)` (the module-level generator the policies'
coins and `random.choice` draw from) and then ONE one-env `interact_environment(env, policy, env_seed=env_seed_i)`; policy and
env share one `Vocabulary` object, as in `llm_rl_scripts/wordle/misc/data_gen.py`, so RandomMixturePolicy's words come from
the env's `random.Random(env_seed)`.  Every episode gets a freshly constructed policy (empty OptimalPolicy cache).

The env is handed to `interact_environment` behind `SameEnvBatched`, a one-env BatchedTextEnv that steps the env object itself.
The reference's own adapter (`TextEnvToBatchedTextEnv.reset`) steps a deepcopy of the env, whose Vocabulary is then no longer the
policy's: the policy's words would come from the unseeded `random.Random()` the env constructor left on the shared Vocabulary, and
no stream would exist to pin.  The shared stream is the contract of this package; policies, env and loop run unmodified.

Per computed OptimalPolicy turn the file records F, `best_words` (the list the policy cached for that state) and
`float.hex(best_info)`; best_info is recomputed here for best_words[0] from the reference's own `game.all_next`, in the
reference's operation order.
"""
from __future__ import annotations

import contextlib
import io
import json
import math
import multiprocessing as mp
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
VOCAB_DIR = os.path.join(ROOT, "lmrl-gym_amd", "data", "vocab")
OUT = os.path.join(HERE, "wordle_scripted_policies.json")


def _words(name):
    return [w.strip() for w in open(os.path.join(VOCAB_DIR, name)) if len(w.strip()) == 5]


def sublist64():
    """64 words of the 431-word list in file order: the three default start words it holds + every 7th word."""
    words = _words("wordle_official_400.txt")
    keep = {words.index(w) for w in ("raise", "audio", "slate")}
    for i in range(0, len(words), 7):
        if len(keep) < 64:
            keep.add(i)
    assert len(keep) == 64
    return [words[i] for i in sorted(keep)]


MIX = lambda p: dict(kind="mixture", prob_smart=p)   # noqa: E731
CASES = [
    dict(name="mixture_p0.0", vocab="wordle_official_400.txt", policy=MIX(0.0), n=64),
    dict(name="mixture_p0.5", vocab="wordle_official_400.txt", policy=MIX(0.5), n=64),
    dict(name="mixture_p1.0", vocab="wordle_official_400.txt", policy=MIX(1.0), n=64),
    dict(name="optimal_start_raise", vocab="wordle_official_400.txt", policy=dict(kind="optimal", start_words=["raise"]), n=48),
    dict(name="optimal_no_start_64", vocab="sublist64", policy=dict(kind="optimal", start_words=None), n=16),
    dict(name="optimal_default_start_64", vocab="sublist64", policy=dict(kind="optimal", start_words="default"), n=16),
    dict(name="coin_optimal_mixture_64", vocab="sublist64",
         policy=dict(kind="coin", prob1=0.5, policy1=dict(kind="optimal", start_words=None), policy2=MIX(0.5)), n=32),
]


def run_case(ci):
    sys.path.insert(0, HERE)
    import _ref_import
    _ref_import.install()
    from LLM_RL.environment import interact_environment
    from llm_rl_scripts.wordle.env import scripted_policies as SP
    from llm_rl_scripts.wordle.env.env import WordleEnvironment
    from llm_rl_scripts.wordle.env.game import Vocabulary, WordleGame

    from LLM_RL.environment import BatchedTextEnv

    class SameEnvBatched(BatchedTextEnv):
        def __init__(self, env):
            self.env = env

        def reset(self, seed=None, options=None):
            return [self.env.reset(seed=seed[0], options=None if options is None else options[0])]

        def step(self, text_history, done=None):
            return [None if (done is not None and done[0]) else self.env.step(text_history[0])]

    case = CASES[ci]
    words = sublist64() if case["vocab"] == "sublist64" else _words(case["vocab"])
    seeder = random.Random(1000 + ci)
    turns_log = []

    def build(spec, vocab):
        if spec["kind"] == "mixture":
            return SP.RandomMixturePolicy(spec["prob_smart"], vocab)
        if spec["kind"] == "coin":
            return SP.MixturePolicy(spec["prob1"], build(spec["policy1"], vocab), build(spec["policy2"], vocab))
        sw = spec["start_words"]
        start = None if sw is None else SP.StartWordPolicy(None if sw == "default" else list(sw))
        if sw == "default":
            spec["start_words_resolved"] = list(start.start_words)
        pol = SP.OptimalPolicy(vocab, start_word_policy=start)
        inner = pol.act

        def act(text_history):
            game = WordleGame.from_str(SP.text_history_to_str(text_history), pol.vocab)
            cached = game.state in pol.cache
            out = inner(text_history)
            if not cached and game.state in pol.cache:
                best_words = list(pol.cache[game.state])
                total_entropy, total = 0.0, 0
                for next_state, state_count in game.all_next(best_words[0]):
                    total_entropy += math.log(next_state.vocab.filtered_vocab_size()) * state_count
                    total += state_count
                best_info = math.log(game.vocab.filtered_vocab_size()) - (total_entropy / total)
                turns_log.append(dict(turn=len(game.action_history), F=game.vocab.filtered_vocab_size(), best_words=best_words,
                                      best_info=float.hex(best_info)))
            return out
        pol.act = act
        return pol

    episodes = []
    t0 = time.time()
    for _ in range(case["n"]):
        env_seed = seeder.randint(0, 2 ** 31 - 1)
        policy_seed = seeder.randint(0, 2 ** 31 - 1)
        vocab = Vocabulary(list(words), None)
        env = WordleEnvironment(vocab)
        policy = build(case["policy"], vocab)
        del turns_log[:]
        random.seed(policy_seed)
        with contextlib.redirect_stdout(io.StringIO()):      # the reference's loop prints every history
            transitions = interact_environment(SameEnvBatched(env), policy, env_seed=env_seed)[0]
        episodes.append(dict(env_seed=env_seed, policy_seed=policy_seed,
                             actions=[t.post_action_history[-1].text for t in transitions],
                             observations=[t.post_transition_history[-1].text for t in transitions],
                             rewards=[float(t.reward) for t in transitions], done=bool(transitions[-1].done),
                             optimal_turns=[dict(t) for t in turns_log]))
    out = dict(name=case["name"], policy=case["policy"], episodes=episodes, ref_seconds=round(time.time() - t0, 2))
    if case["vocab"] == "sublist64":
        out["vocab_words"] = words
    else:
        out["vocab"] = case["vocab"]
    return out


def main():
    with mp.Pool(len(CASES)) as pool:
        cases = pool.map(run_case, range(len(CASES)))
    n_tie = sum(1 for c in cases for ep in c["episodes"] for t in ep["optimal_turns"] if len(t["best_words"]) > 1)
    n_turns = sum(len(ep["optimal_turns"]) for c in cases for ep in c["episodes"])
    with open(OUT, "w") as f:
        json.dump(dict(n_tie_turns=n_tie, n_optimal_turns=n_turns, cases=cases), f, indent=None, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes;", n_turns, "computed turns,", n_tie, "ties;",
          {c["name"]: c["ref_seconds"] for c in cases})


if __name__ == "__main__":
    main()
