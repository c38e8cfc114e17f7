"""Generates tests/golden/offline_rl_data.json: what the reference's offline data path makes of scripted Wordle episodes and of a few
multi-trajectory chains — by RUNNING the reference's own classes (imported from the reference tree through tests/golden/_ref_import.py);
the file holds inputs and results only.

    python tests/golden/make_offline_data_fixture.py

Episodes: a selection of tests/golden/wordle_scripted_policies.json (every length from 1 to 6 turns, words outside the vocabulary, i.e. the
bad-word reward).  Per episode the raw history goes through the reference's `reformat_history` (wordle/env/env.py:7-17), the item / chain map
of train_ilql_gpt2.py:123-134 (reward [0] + [r, 0] per turn), `TokenTrajectoryChain.from_text_trajectory_chain`,
`ILQLData.from_token_trajectory_chain` and `MCData.from_token_trajectory_chain` (`get_rtg` on the numpy stand-in of jax.numpy), with this
package's `WordleTokenizer` as the tokenizer (no GPT-2 tokenizer files exist offline; its ids are GPT-2's).

Chains: synthetic chains of Wordle-alphabet texts, among them a next trajectory without any action and next trajectories whose first action
sits at index 1, through the same three functions per chain link.

Blocking (JaxSeq's `block_sequences`) is not part of the reference tree, so the fixture stores per-item arrays; the blocked forms are pinned
to this package's host `block_sequences` in the tests.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _ref_import  # noqa: E402

_ref_import.install(jnp_shim=True)
from LLM_RL.algorithms.ilql.data import ILQLData  # noqa: E402
from LLM_RL.algorithms.mc_returns.data import MCData  # noqa: E402
from LLM_RL.environment import Text, TextTrajectory, TextTrajectoryChain, TokenTrajectoryChain  # noqa: E402
from llm_rl_scripts.wordle.env.env import reformat_history  # noqa: E402

import lmrl_gym_amd  # noqa: E402,F401
from lmrl_gym_amd.datasets import WordleTokenizer  # noqa: E402

GAMMA = 0.99
OUT = os.path.join(HERE, "offline_rl_data.json")


def fl(a):
    return [float(x) for x in np.asarray(a, dtype=np.float32)]


def token_fields(tt):
    return dict(tokens=[int(x) for x in tt.tokens], is_action=[int(x) for x in tt.is_action], reward=fl(tt.reward), done=bool(tt.done))


def data_fields(chain):
    il = ILQLData.from_token_trajectory_chain(chain)
    out = dict(ilql=dict(should_take_action=[int(x) for x in il.should_take_action], rewards=fl(il.rewards), done=bool(il.done),
                         next_token_ids=None if il.next_token_ids is None else [int(x) for x in il.next_token_ids],
                         next_done=None if il.next_done is None else bool(il.next_done)))
    mc = MCData.from_token_trajectory_chain(chain, GAMMA)
    out["mc"] = dict(should_take_action=[int(x) for x in mc.should_take_action], returns=fl(mc.returns))
    return out


def select_episodes(G):
    picked, per_len, bad = [], {}, 0
    for case in G["cases"]:
        words = set(case["vocab_words"]) if "vocab_words" in case else None
        for i, ep in enumerate(case["episodes"]):
            n = len(ep["actions"])
            has_bad = words is not None and any(a not in words for a in ep["actions"])
            take = i < 2 or per_len.get(n, 0) < 4 or (has_bad and bad < 6)
            if take:
                per_len[n] = per_len.get(n, 0) + 1
                bad += int(has_bad)
                picked.append((case["name"], i, ep, has_bad))
    assert set(per_len) == {1, 2, 3, 4, 5, 6} and bad >= 1
    return picked


def chain_of(trajs):
    """[(texts [(str, is_action)], rewards, done), ...] -> TextTrajectoryChain linked in order"""
    nxt = None
    for texts, rewards, done in reversed(trajs):
        nxt = TextTrajectoryChain(TextTrajectory(tuple(Text(s, bool(a)) for s, a in texts), tuple(rewards), done), nxt)
    return nxt


SYNTHETIC = [
    # three links; the second starts with an observation of one token ('\n'): its first action is at index 1
    [([("Wordle:\n", 0), ("s t a r e\n", 1), ("b y b b g\n", 0)], [0.0, -1.0, 0.0], False),
     ([("\n", 0), ("c l o u d\n", 1), ("b b g b b\n", 0)], [0.0, -1.0, 0.0], False),
     ([("b b g b b\n", 0), ("p i o u s\n", 1), ("g g g g g\n", 0)], [0.0, 0.0, 0.0], True)],
    # the next trajectory has no action at all and is done: all of it is taken, with its done
    [([("Wordle:\n", 0), ("a d i e u\n", 1)], [0.0, -1.0], False),
     ([("b b y b b\n", 0)], [0.0], True)],
    # no action in the next trajectory, not done
    [([("Wordle:\n", 0), ("a d i e u\n", 1)], [0.0, -2.0], False),
     ([("b b y b b\n", 0), ("\n", 0)], [0.0, 0.0], False)],
    # the next trajectory STARTS with an action: index 0 is skipped by the rule (is_action[1:]), the first action found is index 1
    [([("Wordle:\n", 0), ("q u e r y\n", 1), ("b b b y b\n", 0)], [0.0, -1.0, 0.0], False),
     ([("r a i s e\n", 1), ("y b b b b\n", 0)], [-1.0, 0.0], False),
     ([("y b b b b\n", 0), ("t h o r n\n", 1), ("b b b g b\n", 0), ("w o r r y\n", 1)], [0.0, -1.0, 0.0, -10.0], False)],
    # a single link
    [([("Wordle:\n", 0), ("m o u n t\n", 1), ("g g g g g\n", 0)], [0.0, 0.0, 0.0], True)],
]


def main():
    tok = WordleTokenizer()
    with open(os.path.join(HERE, "wordle_scripted_policies.json")) as f:
        G = json.load(f)
    episodes = []
    for name, i, ep, has_bad in select_episodes(G):
        raw = tuple()
        for a, o in zip(ep["actions"], ep["observations"]):
            raw += (Text(a, True), Text(o, False))
        hist = reformat_history(raw)
        reward = [0.0] + sum([[float(r), 0.0] for r in ep["rewards"]], [])
        chain = TextTrajectoryChain(TextTrajectory(hist, tuple(reward), bool(ep["done"])), None)
        tc = TokenTrajectoryChain.from_text_trajectory_chain(chain, tok)
        episodes.append(dict(case=name, index=i, env_seed=ep["env_seed"], policy_seed=ep["policy_seed"], actions=ep["actions"],
                             observations=ep["observations"], rewards=ep["rewards"], bad_word=has_bad,
                             **token_fields(tc.token_trajectory), **data_fields(tc)))
    chains = []
    for trajs in SYNTHETIC:
        tc = TokenTrajectoryChain.from_text_trajectory_chain(chain_of(trajs), tok)
        links, cur = [], tc
        while cur is not None:
            links.append(dict(**token_fields(cur.token_trajectory), **data_fields(cur)))
            cur = cur.next
        chains.append(dict(texts=[dict(texts=[[s, int(a)] for s, a in t], reward=list(r), done=d) for t, r, d in trajs], links=links))
    out = {"_meta": "reference: wordle/env/env.py reformat_history, LLM_RL/environment.py TokenTrajectoryChain.from_text_trajectory_chain, "
                    "ilql/data.py ILQLData.from_token_trajectory_chain, mc_returns/data.py MCData.from_token_trajectory_chain, run on episodes of "
                    "wordle_scripted_policies.json and on synthetic chains (tests/golden/make_offline_data_fixture.py)",
           "gamma": GAMMA, "pad_token_id": tok.pad_token_id, "episodes": episodes, "chains": chains}
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    lens = sorted({len(e["actions"]) for e in episodes})
    print(f"{len(episodes)} episodes (turns {lens}, {sum(e['bad_word'] for e in episodes)} with a word outside the vocabulary), {len(chains)} chains, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
