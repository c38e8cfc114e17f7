"""Scripted Wordle policies and the offline data generator on the MI355X (csrc/wordle_policy.hip).

Public names mirror the reference (`llm_rl_scripts/wordle/env/scripted_policies.py`, `wordle/env/data.py`):
`RandomMixturePolicy`, `OptimalPolicy`, `StartWordPolicy`, `MixturePolicy`, `PolicyDataGenerator`, with the reference's
constructor arguments.  A policy is used two ways:

* as a `BatchedTextPolicy` under `interact_environment` / `text_env_eval`: the knowledge state of every row is rebuilt from the
  history text by the `WordleGame.from_str` rule (game.py:251-271) and `lmrl_wordle_policy_act` chooses the words;
* handed to `WordleScriptedRollouts`, the episode loop that never leaves the device (`lmrl_wordle_policy_episodes`).

Determinism: every episode has an env stream `random.Random(env_seed)` and a policy stream `random.Random(policy_seed)` standing
for the module-level generator the reference's coins and `random.choice` draw from.  RandomMixturePolicy draws its words from the
ENV stream — the wiring of `wordle/misc/data_gen.py`, where policy and env share one Vocabulary object; under
`interact_environment` that needs `policy.attach(env)` with the `VectorWordleEnv` that is stepped.  OptimalPolicy is the reference
policy with an empty cache at the start of every episode.  Not carried over: WrongPolicy, RepeatPolicy, MonteCarloPolicy,
UserPolicy.
"""
from __future__ import annotations

import ctypes
import math
import random
from typing import Any, Dict, Iterator, List, Optional, Sequence, Union

import numpy as np

from .. import _lib
from ..environment import BatchedTextPolicy, Text, TextHistory, TextTrajectory
from . import wordle as W

MAX_START_WORDS = 64
KIND_MIXTURE, KIND_OPTIMAL = 0, 1
# StartWordPolicy's default list (scripted_policies.py:49-53)
DEFAULT_START_WORDS = ["opera", "tears", "soare", "roate", "raise", "arose", "earls", "laser", "reals", "aloes", "reais", "slate", "sauce",
                       "slice", "shale", "saute", "share", "sooty", "shine", "suite", "crane", "adieu", "audio", "stare", "roast", "ratio",
                       "arise", "tales"]


class _Leaf(ctypes.Structure):             # lmrl_wordle_policy_leaf (include/lmrl_amd.h)
    _fields_ = [("kind", ctypes.c_int32), ("n_start", ctypes.c_int32), ("start_off", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("prob_smart", ctypes.c_double)]


class PolicyDesc(ctypes.Structure):        # lmrl_wordle_policy_desc
    _fields_ = [("coin", ctypes.c_int32), ("pad_", ctypes.c_int32), ("prob1", ctypes.c_double), ("leaf", _Leaf * 2),
                ("start_words", ctypes.c_uint32 * MAX_START_WORDS)]


def _as_vocab(vocab) -> W.Vocabulary:
    return W.Vocabulary.from_file(vocab) if isinstance(vocab, str) else vocab


def log_table(n_words: int) -> np.ndarray:
    """logtab[k] = math.log(k), the function the reference calls (scripted_policies.py:88-90); entry 0 is never read."""
    return np.array([-math.inf] + [math.log(k) for k in range(1, n_words + 1)], dtype=np.float64)


def packed_vocab(vocab: W.Vocabulary) -> np.ndarray:
    return np.array([W.pack_guess(w) for w in vocab.all_vocab], dtype=np.uint32)


def _u32p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


# --------------------------------------------------------------------------------------------- state from text
def obs_code(transition: str) -> int:
    """'<g><y><b>...' -> the observation code of `lmrl_wordle_step` (3 bits per symbol, count in bits 16-18)."""
    syms = [transition[i:i + 3] for i in range(0, len(transition), 3)]
    code = 0
    for k, s in enumerate(syms):
        code |= {"<g>": 1, "<y>": 2, "<b>": 3}[s] << (3 * k)
    return code | (len(syms) << 16)


def state_from_history(raw_history: TextHistory, vocab: W.Vocabulary, require_words_in_vocab: bool = True):
    """`WordleGame.from_str` (game.py:251-271) on a raw-format history: actions that are not 5 letters a-z (or not vocabulary words)
    are skipped, every other one applies its transition string.  Returns (masks uint32[10] = forb[5] + must[5], n_actions)."""
    L = _lib.lib()
    items = list(raw_history)
    assert len(items) <= 2 * W.N_TRIES, "Too many transitions"
    actions, transitions = items[::2], items[1::2]
    assert len(actions) == len(transitions), "number of actions and transitions do not match"
    masks = np.zeros(10, dtype=np.uint32)
    for a, tr in zip(actions, transitions):
        g = W.pack_guess(a.text)
        if g == W.BAD_GUESS or (require_words_in_vocab and a.text not in vocab):
            continue
        if L.lmrl_wordle_policy_host_apply_feedback(_u32p(masks), g, obs_code(tr.text)) != 0:
            raise NotImplementedError(f"transition {tr.text!r} does not hold five <g>/<y>/<b> symbols")
    return masks, len(actions)


# --------------------------------------------------------------------------------------------- policies
class _ScriptedPolicy(BatchedTextPolicy):
    """Common text face: rows -> state buffer -> `lmrl_wordle_policy_act` -> action text."""
    reformat = False          # True: histories are in the LM-facing format of ReformatWordleEnvironment

    def _leaves(self):
        raise NotImplementedError

    def _vocab(self) -> W.Vocabulary:
        raise NotImplementedError

    def descriptor(self) -> PolicyDesc:
        d = PolicyDesc()
        spec = self._leaves()
        d.coin, d.prob1 = (1, float(spec[0])) if len(spec) == 3 else (0, 0.0)
        off = 0
        for i, leaf in enumerate(spec[-2:] if len(spec) == 3 else spec):
            kind, prob, start = leaf
            d.leaf[i].kind, d.leaf[i].prob_smart = kind, float(prob)
            d.leaf[i].start_off, d.leaf[i].n_start = off, len(start)
            if off + len(start) > MAX_START_WORDS:
                raise ValueError(f"at most {MAX_START_WORDS} start words fit a device policy descriptor")
            for w in start:
                p = W.pack_guess(w)
                if p == W.BAD_GUESS:
                    raise ValueError(f"start word {w!r} is not five letters a-z")
                d.start_words[off] = p
                off += 1
        return d

    # -- streams of the text face
    def attach(self, env: "W.VectorWordleEnv") -> "_ScriptedPolicy":
        """Draw RandomMixturePolicy's words from `env`'s own streams (policy and env sharing one Vocabulary in the reference)."""
        self._env = env
        self.reformat = env.reformat
        return self

    def seed(self, policy_seeds: Sequence[int]) -> "_ScriptedPolicy":
        """One policy stream `random.Random(seed)` per row of the batches that follow."""
        self._policy_seeds = [W._seed_magnitude(s) for s in policy_seeds]
        self._mt_pol = None
        return self

    def _device(self, n: int):
        import torch as t
        dev = _lib.require_gpu()
        L = _lib.lib()
        vocab = self._vocab()
        if getattr(self, "_dev_n", None) != n:
            self._own_env = W.VectorWordleEnv(vocab, reformat=False) if getattr(self, "_own_env", None) is None else self._own_env
            V = len(vocab.all_vocab)
            self._scratch = t.zeros(L.lmrl_wordle_policy_scratch_bytes(n, V), dtype=t.uint8, device=dev)
            self._logtab = t.from_numpy(log_table(V)).to(dev)
            self._mt_own = None
            self._mt_pol = None
            self._dev_n = n
        def streams(seeds):
            mt = t.zeros(L.lmrl_mt_bytes(n), dtype=t.uint8, device=dev)
            sd = t.from_numpy(np.asarray(seeds, dtype=np.uint64).view(np.int64).copy()).to(dev)
            _lib.check(L.lmrl_mt_seed(_lib.ptr(mt), _lib.ptr(sd), None, n, _lib.stream_ptr()), "lmrl_mt_seed")
            return mt
        if self._mt_pol is None:
            seeds = list(getattr(self, "_policy_seeds", None) or [])
            seeds = (seeds + [W._seed_magnitude(None) for _ in range(n - len(seeds))])[:n]      # unseeded rows: OS entropy, like `random`
            self._mt_pol = streams(seeds)
        env = getattr(self, "_env", None)
        if env is not None and env.n == n:
            mt_env = env.mt
        else:                                     # a Vocabulary of the policy's own: `random.Random()` (game.py:159-161)
            if self._mt_own is None:
                self._mt_own = streams([W._seed_magnitude(None) for _ in range(n)])
            mt_env = self._mt_own
        return dev, L, mt_env

    def act(self, text_history, done=None):
        import torch as t
        n = len(text_history)
        if done is None:
            done = [False] * n
        vocab = self._vocab()
        state = np.zeros((W.N_TRIES + 13, n), dtype=np.uint32)
        active = np.zeros(n, dtype=np.uint8)
        for i, (h, d) in enumerate(zip(text_history, done)):
            if d or h is None:
                continue
            raw = W.deformat_history(h) if self.reformat else tuple(h)
            masks, n_actions = state_from_history(raw, vocab)
            state[:10, i] = masks
            state[11, i] = n_actions
            active[i] = 1
        dev, L, mt_env = self._device(n)
        state_d = t.from_numpy(state.view(np.int32)).to(dev)
        active_d = t.from_numpy(active).to(dev)
        guess_d = t.full((n,), -1, dtype=t.int32, device=dev)
        desc = self.descriptor()
        _lib.check(L.lmrl_wordle_policy_act(self._own_env._ctx, ctypes.byref(desc), _lib.ptr(state_d), _lib.ptr(mt_env), _lib.ptr(self._mt_pol),
                                            _lib.ptr(active_d), _lib.ptr(self._logtab), _lib.ptr(self._scratch), self._scratch.numel(),
                                            _lib.ptr(guess_d), None, None, None, n, _lib.stream_ptr()), "lmrl_wordle_policy_act")
        guess = guess_d.cpu().numpy().view(np.uint32)
        out: List[Optional[TextHistory]] = []
        for i, h in enumerate(text_history):
            if not active[i]:
                out.append(None)
                continue
            if int(guess[i]) == W.BAD_GUESS:
                raise IndexError("Cannot choose from an empty sequence (no vocabulary word is consistent with the history)")
            word = W.unpack_word(int(guess[i]))
            out.append(tuple(h) + (Text(" ".join(word) + "\n" if self.reformat else word, True),))
        return out


class RandomMixturePolicy(_ScriptedPolicy):
    """With probability `prob_smart` a uniformly random word still consistent with the feedback, else a uniformly random vocabulary
    word (scripted_policies.py:114-126)."""

    def __init__(self, prob_smart: float, vocab: Union[str, W.Vocabulary]):
        self.vocab = _as_vocab(vocab)
        self.prob_smart = prob_smart

    def _vocab(self):
        return self.vocab

    def _leaves(self):
        return [(KIND_MIXTURE, self.prob_smart, [])]


class StartWordPolicy(_ScriptedPolicy):
    """A random start word still consistent with the history, judged on the start words alone (scripted_policies.py:42-64).  On the device
    it is the first-turn policy of `OptimalPolicy`; used on its own it is host code on one `random.Random` per row."""

    def __init__(self, start_words: Optional[List[str]] = None):
        self.start_words = list(DEFAULT_START_WORDS) if start_words is None else list(start_words)
        self.vocab = W.Vocabulary(self.start_words)
        self._rngs: List[random.Random] = []

    def seed(self, policy_seeds):
        self._rngs = [random.Random(s) for s in policy_seeds]
        return self

    def attach(self, env):
        self.reformat = env.reformat
        return self

    def act(self, text_history, done=None):
        L = _lib.lib()
        n = len(text_history)
        if done is None:
            done = [False] * n
        while len(self._rngs) < n:
            self._rngs.append(random.Random())
        words = packed_vocab(self.vocab)
        out = []
        for i, (h, d) in enumerate(zip(text_history, done)):
            if d or h is None:
                out.append(None)
                continue
            raw = W.deformat_history(h) if self.reformat else tuple(h)
            masks, _ = state_from_history(raw, self.vocab)
            idx = np.zeros(len(words), dtype=np.int32)
            f = L.lmrl_wordle_policy_host_filtered(_u32p(words), len(words), _u32p(masks), _u32p(idx))
            rng = self._rngs[i]
            word = self.start_words[int(idx[rng._randbelow(f)])] if f > 0 else "".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(W.N_CHARS))
            out.append(tuple(h) + (Text(" ".join(word) + "\n" if self.reformat else word, True),))
        return out


class OptimalPolicy(_ScriptedPolicy):
    """The information-gain player (scripted_policies.py:66-96): among the words still consistent with the feedback, one of those with the
    largest expected log-reduction of the consistent set; `start_word_policy` answers the first turn instead."""

    def __init__(self, vocab: Union[str, W.Vocabulary], start_word_policy: Optional[StartWordPolicy] = None, progress_bar: bool = False):
        self.vocab = _as_vocab(vocab)
        if start_word_policy is not None and not isinstance(start_word_policy, StartWordPolicy):
            raise TypeError("the device OptimalPolicy takes a StartWordPolicy (or None) as start_word_policy")
        if start_word_policy is not None and not start_word_policy.start_words:
            raise ValueError("StartWordPolicy with an empty word list")
        self.start_word_policy = start_word_policy
        self.progress_bar = progress_bar

    def _vocab(self):
        return self.vocab

    def _leaves(self):
        return [(KIND_OPTIMAL, 0.0, self.start_word_policy.start_words if self.start_word_policy is not None else [])]


class MixturePolicy(_ScriptedPolicy):
    """A coin between two policies per turn (scripted_policies.py:143-153); both are RandomMixturePolicy / OptimalPolicy objects over one
    vocabulary."""

    def __init__(self, prob1: float, policy1: _ScriptedPolicy, policy2: _ScriptedPolicy):
        for p in (policy1, policy2):
            if not isinstance(p, (RandomMixturePolicy, OptimalPolicy)):
                raise TypeError("the device MixturePolicy mixes RandomMixturePolicy / OptimalPolicy objects")
        if policy1.vocab.all_vocab != policy2.vocab.all_vocab:
            raise ValueError("MixturePolicy: both policies must play on the same vocabulary")
        self.prob1, self.policy1, self.policy2 = prob1, policy1, policy2

    def _vocab(self):
        return self.policy1.vocab

    def _leaves(self):
        return [self.prob1, self.policy1._leaves()[0], self.policy2._leaves()[0]]


# --------------------------------------------------------------------------------------------- the device loop
class ScriptedRecords:
    """Host copy of one batch of episodes: guess / obs uint32[6][N], reward float32[6][N], flags uint8[6][N], n_turns int32[N]."""

    def __init__(self, guess, obs, reward, flags, n_turns, env_seeds, policy_seeds, bad_word_reward):
        self.guess, self.obs, self.reward, self.flags, self.n_turns = guess, obs, reward, flags, n_turns
        self.env_seeds, self.policy_seeds, self.bad_word_reward = env_seeds, policy_seeds, bad_word_reward

    def __len__(self):
        return len(self.n_turns)

    def episode(self, i: int):
        """(actions, raw observations, rewards, done) of episode i, in the raw format of `WordleEnvironment`."""
        k = int(self.n_turns[i])
        actions = [W.unpack_word(int(self.guess[t, i])) for t in range(k)]
        obs = [W.transition_text(int(self.obs[t, i])) for t in range(k)]
        rewards = [float(self.reward[t, i]) for t in range(k)]
        return actions, obs, rewards, bool(self.flags[k - 1, i] & 1)

    def to_items(self) -> List[Dict[str, Any]]:
        """jsonl items of `wordle/misc/data_gen.py:53-62`: the reformatted history, `[r, 0.0]` per turn (data.py:31), done."""
        from ..datasets import text_trajectory_to_item
        items = []
        for i in range(len(self)):
            actions, obs, rewards, done = self.episode(i)
            raw: TextHistory = tuple()
            for a, o in zip(actions, obs):
                raw += (Text(a, True), Text(o, False))
            items.append(text_trajectory_to_item(W.reformat_history(raw), sum([[r, 0.0] for r in rewards], []), done))
        return items

    def to_trajectories(self) -> List[TextTrajectory]:
        out = []
        for i in range(len(self)):
            actions, obs, rewards, done = self.episode(i)
            raw: TextHistory = tuple()
            for a, o in zip(actions, obs):
                raw += (Text(a, True), Text(o, False))
            out.append(TextTrajectory(raw, tuple(sum([[r, 0.0] for r in rewards], [])), done))
        return out

    def summary(self) -> Dict[str, Dict[str, Any]]:
        """The summary `text_env_eval` returns (environment.py:257-298)."""
        rewards = self.reward.sum(axis=0, dtype=np.float64).astype(np.float32)
        dones = np.array([self.flags[int(k) - 1, i] & 1 for i, k in enumerate(self.n_turns)], dtype=np.float32)

        def _summary(x):
            return dict(mean=np.mean(x), std=np.std(x), min=np.min(x), max=np.max(x))
        return dict(reward=_summary(rewards), done=_summary(dones), length=_summary(np.asarray(self.n_turns)))


class WordleScriptedRollouts:
    """`bsize` episodes of a scripted policy per `run`: reset, then up to six (act, step) turns with per-env done masking, all on the
    device and on one stream (`lmrl_wordle_policy_episodes`); every buffer belongs to this object."""

    def __init__(self, vocab: W.Vocabulary, policy: _ScriptedPolicy, bsize: int, require_words_in_vocab: bool = True,
                 bad_word_reward: float = -1.0):
        import torch as t
        if isinstance(policy, StartWordPolicy) or not isinstance(policy, _ScriptedPolicy):
            raise TypeError("WordleScriptedRollouts takes a RandomMixturePolicy, OptimalPolicy or MixturePolicy")
        if policy._vocab().all_vocab != vocab.all_vocab:
            raise ValueError("policy and env must play on the same vocabulary")
        self.vocab, self.policy, self.n = vocab, policy, int(bsize)
        self.env = W.VectorWordleEnv(vocab, require_words_in_vocab, bad_word_reward, reformat=False)
        self.dev, self._L, n, V = self.env.device, self.env._L, self.n, len(vocab.all_vocab)
        L = self._L
        self.desc = policy.descriptor()
        z = lambda *shape, dtype: t.zeros(*shape, dtype=dtype, device=self.dev)   # noqa: E731
        self.state = z(L.lmrl_wordle_state_bytes(n), dtype=t.uint8)
        self.mt_env, self.mt_pol = z(L.lmrl_mt_bytes(n), dtype=t.uint8), z(L.lmrl_mt_bytes(n), dtype=t.uint8)
        self.scratch = z(L.lmrl_wordle_policy_scratch_bytes(n, V), dtype=t.uint8)
        self.logtab = t.from_numpy(log_table(V)).to(self.dev)
        self.active = z(n, dtype=t.uint8)
        self.env_seeds, self.pol_seeds = z(n, dtype=t.int64), z(n, dtype=t.int64)
        self.guess, self.obs = z((W.N_TRIES, n), dtype=t.int32), z((W.N_TRIES, n), dtype=t.int32)
        self.reward, self.flags = z((W.N_TRIES, n), dtype=t.float32), z((W.N_TRIES, n), dtype=t.uint8)
        self.n_turns = z(n, dtype=t.int32)
        self.graph = None

    def _launch(self):
        L = self._L
        p = _lib.ptr
        _lib.check(L.lmrl_wordle_policy_episodes(self.env._ctx, ctypes.byref(self.desc), p(self.state), p(self.mt_env), p(self.mt_pol),
                                                 p(self.env_seeds), p(self.pol_seeds), p(self.logtab), p(self.scratch), self.scratch.numel(),
                                                 p(self.active), p(self.guess), p(self.obs), p(self.reward), p(self.flags), p(self.n_turns),
                                                 self.n, _lib.stream_ptr()), "lmrl_wordle_policy_episodes")

    def capture(self):
        """The whole batch of episodes as one hipGraph (`run_device(..., use_graph=True)` replays it); one eager run warms it first."""
        import torch as t
        self._launch()
        t.cuda.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, capture_error_mode="thread_local"):
            self._launch()
        self.graph = g
        return g

    def run_device(self, env_seeds, policy_seeds, use_graph: bool = False) -> None:
        """Seeds (numpy / list, or int64 device tensors of length bsize) in, records left on the device; no host sync."""
        import torch as t
        for dst, src in ((self.env_seeds, env_seeds), (self.pol_seeds, policy_seeds)):
            if not isinstance(src, t.Tensor):
                src = t.from_numpy(np.array([W._seed_magnitude(int(s)) for s in src], dtype=np.uint64).view(np.int64))
            assert src.numel() == self.n, "one env seed and one policy seed per episode of the batch"
            dst.copy_(src, non_blocking=True)
        if use_graph:
            if self.graph is None:
                self.capture()
            self.graph.replay()
        else:
            self._launch()

    def records(self, n: Optional[int] = None) -> ScriptedRecords:
        n = self.n if n is None else n
        u32 = lambda x: x.cpu().numpy().view(np.uint32)[:, :n].copy()   # noqa: E731
        rec = ScriptedRecords(u32(self.guess), u32(self.obs), self.reward.cpu().numpy()[:, :n].copy(), self.flags.cpu().numpy()[:, :n].copy(),
                              self.n_turns.cpu().numpy()[:n].copy(), self.env_seeds.cpu().numpy()[:n].copy(),
                              self.pol_seeds.cpu().numpy()[:n].copy(), self.env.bad_word_reward)
        if (rec.flags & 8).any():
            raise IndexError("Cannot choose from an empty sequence (filtered vocabulary is empty)")
        return rec

    def token_records(self, n: Optional[int] = None, tokens=None, cap: Optional[int] = None):
        """The first `n` episodes of the last `run_device` as `algorithms.ppo_device.PPORecords` (`lmrl_wordle_tok_scripted_records`): the rows
        `to_items()` followed by the tokenizer would give (reformatted history, reward on the newline closing each action), built from the
        resident record buffers; no token data visits the host.  tokens: a `rollout.WordleTokenTable` (default: GPT-2 ids); cap: row pitch
        (default: the longest possible episode).  One 4-byte readback reports episodes whose policy ran out of words, as `records()` does."""
        import torch as t
        from ..algorithms.ppo_device import PPORecords
        from ..rollout import WordleTokenTable
        tokens = tokens or WordleTokenTable.default_gpt2()
        n = self.n if n is None else int(n)
        assert 0 < n <= self.n
        cap = len(tokens.header) + W.N_TRIES * 12 if cap is None else int(cap)
        tok = t.empty((n, cap), dtype=t.int32, device=self.dev)
        ia = t.empty((n, cap), dtype=t.uint8, device=self.dev)
        rw = t.empty((n, cap), dtype=t.float32, device=self.dev)
        n_tok, done = t.empty(n, dtype=t.int32, device=self.dev), t.empty(n, dtype=t.uint8, device=self.dev)
        err = t.empty(1, dtype=t.int32, device=self.dev)
        ct = tokens.c_struct()
        p = _lib.ptr
        _lib.check(self._L.lmrl_wordle_tok_scripted_records(ctypes.byref(ct), p(self.guess), p(self.obs), p(self.reward), p(self.flags), p(self.n_turns),
                                                            self.n, n, cap, p(tok), p(ia), p(rw), p(n_tok), p(done), p(err), _lib.stream_ptr()),
                   "lmrl_wordle_tok_scripted_records")
        if int(err.cpu().numpy()[0]):
            raise IndexError("Cannot choose from an empty sequence (filtered vocabulary is empty), or an episode does not fit the row pitch")
        return PPORecords(tok, ia, rw, n_tok, done)

    def run(self, env_seeds, policy_seeds, use_graph: bool = False) -> ScriptedRecords:
        """Fewer seeds than bsize: the batch is padded with repeats of the last episode and the records cut back."""
        env_seeds, policy_seeds = list(env_seeds), list(policy_seeds)
        k = len(env_seeds)
        assert 0 < k <= self.n and len(policy_seeds) == k
        pad = self.n - k
        self.run_device(env_seeds + [env_seeds[-1]] * pad, policy_seeds + [policy_seeds[-1]] * pad, use_graph=use_graph)
        return self.records(k)

    def close(self):
        self.env.close()


# --------------------------------------------------------------------------------------------- data generator
class PolicyDataGenerator:
    """Iterator of `TextTrajectory` (raw history, `[r, 0.0]` per turn, done) with the reference's env-seed sequence
    `random.Random(seed).randint(0, 2**31 - 1)` (data.py:9-34).  Episode k's policy stream is seeded with the k-th
    `randint(0, 2**31 - 1)` of `random.Random(seed + 1)` (an unseeded generator when seed is None): the reference's module-level generator
    is unseeded, so this sequence is this package's own.  Episodes are produced `bsize` at a time on `WordleScriptedRollouts`."""

    def __init__(self, env, policy: _ScriptedPolicy, seed: Optional[int] = None, bsize: int = 256):
        self.env, self.policy = env, policy
        self.rng = random.Random(seed)
        self.policy_rng = random.Random(None if seed is None else seed + 1)
        self._loop = WordleScriptedRollouts(env.vocab, policy, bsize, env.require_words_in_vocab, env.bad_word_reward)
        self._ready: List[TextTrajectory] = []
        self.last_seeds: List[int] = []

    def __iter__(self) -> Iterator[TextTrajectory]:
        return self

    def next_records(self, n: Optional[int] = None) -> ScriptedRecords:
        n = self._loop.n if n is None else n
        env_seeds = [self.rng.randint(0, 2 ** 31 - 1) for _ in range(n)]
        pol_seeds = [self.policy_rng.randint(0, 2 ** 31 - 1) for _ in range(n)]
        return self._loop.run(env_seeds, pol_seeds)

    def __next__(self) -> TextTrajectory:
        if not self._ready:
            self._ready = self.next_records().to_trajectories()[::-1]
        return self._ready.pop()

    def close(self):
        self._loop.close()
