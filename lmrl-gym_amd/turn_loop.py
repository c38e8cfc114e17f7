"""What the device-resident turn loops share: `TurnLoopEngine`, the base of `MazeRolloutEngine`, `ChessRolloutEngine` and
`TwentyQuestionsRolloutEngine`, and the host helpers that `WordleRolloutEngine` and the generic policies use as well.

An engine supplies its env's side of a turn (`_turn`: prompt feeding, the env step, the record), its episode reset and its host views
(`ppo_records`, `interactions`); the base owns the decode loop between them (steered sampling, `lmrl_gen_accept`, the one-token forwards), the
scripted-steering table and its device-side turn counter, graph capture, the episode's turn loop with its early-exit peeks, in-place weight
loading, and the PPO data round (`ppo_rollouts`) and one-lane `text_env_eval` over ceil(n / B) episode batches.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from . import _lib
from .gpt2 import GPT2Engine, SampleParams


def decode_generation(tokenizer, ids: List[int], eos: Optional[int] = None) -> str:
    """`tokenizer.decode(ids, skip_special_tokens=True)`, the ids cut behind the first `eos` (None: no cut).  Minimal tokenizers without the
    keyword: drop what THEY declare special (`all_special_ids`; default: only the pad id — an eos id is ordinary text unless the tokenizer
    says otherwise, exactly as '\\n' is for the GPT-2 tokenizer)."""
    if eos is not None and eos in ids:
        ids = ids[: ids.index(eos) + 1]
    try:
        return tokenizer.decode(ids, skip_special_tokens=True)
    except TypeError:
        special = getattr(tokenizer, "all_special_ids", None)
        if special is None:
            special = [t for t in (getattr(tokenizer, "pad_token_id", None),) if t is not None]
        special = set(special)
        return tokenizer.decode([t for t in ids if t not in special])


def summarize(x):
    """One field of `text_env_eval`'s summary (LLM_RL/environment.py:211-267)."""
    return dict(mean=np.mean(x), std=np.std(x), min=np.min(x), max=np.max(x))


def round_seeds(B: int, actual: int, seed_generator, draw: bool = True) -> list:
    """The env seeds of one episode batch: `actual` values of `seed_generator` (None: drawn from numpy's global stream, or zeros without `draw`),
    0 for the idle envs of a partial last batch."""
    seeds = [0] * B
    if seed_generator is not None:
        seeds[:actual] = [next(seed_generator) for _ in range(actual)]
    elif draw:
        seeds[:actual] = np.random.randint(0, 2 ** 31 - 1, size=actual).tolist()
    return seeds


def steer_script(id_rows, T: int, max_new: int, B: int, dev, strength: float):
    """The scripted-steering state of an engine: (steer ids int32 [T + slack][max_new][B], turn counter int32 [1], this turn's rows [max_new][B],
    strength).  `id_rows` [T][B] of id lists (cut to `max_new`) or None (no steering: -1).  The slack rows stay -1: capture warm-ups advance the
    counter too."""
    import torch
    steer = np.full((T + 4 * T + 8, max_new, B), -1, dtype=np.int32)
    for ti, row in enumerate(id_rows):
        for b, ids in enumerate(row):
            if ids is not None:
                ids = list(ids)[:max_new]
                steer[ti, : len(ids), b] = ids
    return (torch.from_numpy(steer).to(dev), torch.zeros(1, dtype=torch.int32, device=dev),
            torch.full((max_new, B), -1, dtype=torch.int32, device=dev), float(strength))


def finish_ppo_round(parts, kls, use_advantage_whitening: bool):
    """The per-batch PPO data of one round -> (DevicePPODataset over all of it, all_kls): advantages whitened ONCE over the action tokens of the
    whole round (ppo/base_interface.py:609-615 whitens over every chain handed to the call)."""
    import torch
    from . import dist as D
    from .algorithms.ppo_device import DevicePPODataset
    ds = DevicePPODataset.concat(parts)
    if use_advantage_whitening:
        adv = ds.old_advantages
        ds.old_advantages = D.whiten_distributed(adv.view(-1), ds.should_take_action.view(-1), shift_mean=True).view(adv.shape)
    return ds, (kls[0] if len(kls) == 1 else torch.cat(kls))


class TurnLoopEngine:
    """B lock-step episodes of a text env driven by a GPT-2 policy on one GPU.  A subclass sets `eng, tok, B, T, max_new, eos, pad, dev, _L`, its
    sessions and `traj` (with `live`), calls `_alloc_turn_loop()`, and supplies `_turn`, `run_episode`, `ppo_records`, `interactions`,
    `_graphs` / `_recapture` (its captured turns) and `_round_stats` / `_SUMMARY` (its summary)."""

    _script = None              # `steer_script(...)`, or None
    _POLICY = "policy"          # what `load_params`' message calls the engine
    _DRAW_SEEDS = True          # no seed generator: draw env seeds (False: zeros — the env's reset ignores them)
    _SUMMARY = (("reward", 0, np.float32), ("done", 1, np.float32), ("length", 2, np.int64))      # summary key <- (row of `_round_stats`, dtype)

    def _alloc_turn_loop(self):
        import torch
        z = lambda n: torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.chunk_tok, self.chunk_cnt = z(self.B * 16), z(self.B)
        self.next_tok, self.next_cnt = z(self.B), z(self.B)
        self.epoch = z(1)               # 4th Philox counter word of the sampler: (episode << 12) + turn, advanced on the device (graph replays too)
        self.episodes = 0               # episode batches run by text_env_eval / ppo_rollouts so far: successive calls draw fresh sampler noise
        self._script = None

    # ---- scripted steering ---------------------------------------------------------------------------------------------------------------
    def _set_script(self, id_rows, strength: float):
        self._script = None if id_rows is None else steer_script(id_rows, self.T, self.max_new, self.B, self.dev, strength)

    def _steer_rows(self):
        """This turn's steer rows: row `turn counter` of the scripted table (a device-side index: the same launch in every replay)."""
        s = self._script
        if s is not None:
            _lib.check(self._L.lmrl_gather_rows_bytes(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 1, self.max_new * self.B * 4, _lib.stream_ptr()),
                       "lmrl_gather_rows_bytes")
        return s

    def _end_turn(self, script):
        self.epoch.add_(1)
        if script is not None:
            script[1].add_(1)

    def _start_episode_counters(self, episode: int):
        self.epoch.fill_(int(episode) << 12)
        if self._script is not None:
            self._script[1].zero_()

    # ---- the decode loop -----------------------------------------------------------------------------------------------------------------
    def _generate(self, ses, forward, temperature, top_k, top_p, seed, beta, epoch, active, out_tok, out_len, next_tok, next_cnt, eos, cap,
                  script=None, logits_out=None, q_hook=None):
        """<= `cap` tokens per env from `ses`: sample (steered by `script`'s rows of this turn; `q_hook()` -> the (q1, q2) operands of a value
        policy, per step) | accept into out_tok / out_len, eos (< 0: none) or `cap` ends an env | forward the accepted ids through `forward`."""
        L, sp, ck = self._L, _lib.stream_ptr(), _lib.check
        steer, strength = (script[2], script[3]) if script is not None else (None, 0.0)
        ptrs = [_lib.ptr(x) for x in (active, out_tok, out_len, next_tok, next_cnt)]
        q1 = q2 = None
        for k in range(cap):
            p = SampleParams(temperature, top_k, seed, k, strength, beta, self.pad, epoch, top_p)
            if q_hook is not None:
                q1, q2 = q_hook()
            ses.sample(p, steer_tok=steer[k] if steer is not None else None, active=active, logits_out=logits_out, q1=q1, q2=q2, want_logprob=False)
            ck(L.lmrl_gen_accept(_lib.ptr(ses.token), *ptrs, eos, cap, self.B, sp), "lmrl_gen_accept")
            if k < cap - 1:
                for s in forward:
                    s.forward(next_tok, next_cnt, 1)

    # ---- graphs --------------------------------------------------------------------------------------------------------------------------
    def _new_logits(self, top_k, top_p=0.0):
        """The materialised-logits operand of the warpers (None without them)."""
        import torch
        return torch.empty(self.B, self.eng.cfg.vocab_padded, dtype=torch.float32, device=self.dev) if (top_k > 0 or top_p > 0.0) else None

    def _begin_capture(self, temperature, top_k, top_p, sample_seed):
        self._graph_args = (temperature, top_k, top_p, sample_seed)
        self._logits = self._new_logits(top_k, top_p)

    def _capture(self, *turn_args, **turn_kw):
        """`self._turn(...)` once eagerly (warm-up: allocations, lazy workspaces), then captured -> the graph."""
        import torch
        self._turn(*turn_args, **turn_kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._turn(*turn_args, **turn_kw)
        return g

    def _episode_logits(self, use_graph, temperature, top_k, top_p, sample_seed):
        """The logits operand of an episode's turns; `use_graph`: captures first when nothing is captured or the sampling arguments changed."""
        if not use_graph:
            return self._new_logits(top_k, top_p)
        if not self._graphs() or self._graph_args != (temperature, top_k, top_p, sample_seed):
            self._recapture(temperature, top_k, top_p, sample_seed)
        return self._logits

    # ---- an episode's turns --------------------------------------------------------------------------------------------------------------
    def _run_turns(self, turn, sync_every: int, max_turns: Optional[int]):
        """`turn(i)` for the episode's turns; the host peeks at the live flags every `sync_every` turns to stop early (0: never)."""
        n = self.T if max_turns is None else min(self.T, max_turns)
        for i in range(n):
            if sync_every and i and i % sync_every == 0 and not bool(self.traj["live"].any().item()):
                break
            turn(i)
        return self.traj

    # ---- weights -------------------------------------------------------------------------------------------------------------------------
    def load_params(self, params) -> None:
        """The trainer's fp32 parameters into the policy engine IN PLACE (`GPT2Engine.load_params`: captured turns stay valid, they read the same
        weight buffers).  bf16 policy engines only: a `GPT2EngineF32` policy is rebuilt from the trained weights and handed to `set_params`."""
        if not isinstance(self.eng, GPT2Engine):
            raise _lib.LmrlError(f"{type(self).__name__}.load_params: in-place loading needs a bf16 GPT2Engine {self._POLICY}, not a "
                                 f"{type(self.eng).__name__} (build an engine from the new weights and call set_params)")
        self.eng.load_params(params)
        self._after_weights()

    def _after_weights(self):
        """What else the new weights invalidate (Maze: lane twins, the prefix cache)."""

    # ---- rounds of episode batches -------------------------------------------------------------------------------------------------------
    def _round_seeds(self, actual: int, seed_generator):
        return round_seeds(self.B, actual, seed_generator, self._DRAW_SEEDS)

    def _round_episode(self, seeds, env_options, actual: int, **run_kw):
        return self.run_episode(seeds, env_options, episode=self.episodes, n_live=actual, **run_kw)

    def ppo_data(self, inference, *, gamma: float, lam: float, kl_weight: float, max_length: Optional[int] = None, n: Optional[int] = None, **kw):
        """`ppo_dataset_loader` of the online script on the episodes this engine just ran -> (DevicePPODataset, all_kls): see
        `algorithms.ppo_device.ppo_data_from_records`."""
        from .algorithms.ppo_device import ppo_data_from_records
        return ppo_data_from_records(inference, self.ppo_records(n), gamma=gamma, lam=lam, kl_weight=kl_weight, max_length=max_length, **kw)

    def _ppo_round(self, inference, n_rollouts: int, seed_generator, env_options, use_advantage_whitening: bool, run_kw: dict, data_kw: dict):
        """`ppo_rollouts`: per episode batch the lock-step episode (`run_kw`: its sampling arguments), then its PPO data (`data_kw`) while the record
        is in the engine's buffers -> (dataset, all_kls, summary from the per-env counters: no text is built)."""
        parts, kls, stats = [], [], []
        launched = 0
        while launched < n_rollouts:
            actual = min(n_rollouts - launched, self.B)
            self._round_episode(self._round_seeds(actual, seed_generator), env_options, actual, **run_kw)
            self.episodes += 1
            launched += actual
            ds, kl = self.ppo_data(inference, n=actual, use_advantage_whitening=False, **data_kw)
            parts.append(ds); kls.append(kl)
            stats.append(self._round_stats(actual))
        ds, all_kls = finish_ppo_round(parts, kls, use_advantage_whitening)
        st = np.concatenate(stats, axis=1)
        return ds, all_kls, {name: summarize(st[row].astype(dt)) for name, row, dt in self._SUMMARY}

    def _eval_round(self, n_rollouts: int, seed_generator, env_options, interaction_callback, run_kw: dict):
        """One-lane `text_env_eval`: ceil(n / B) episode batches -> their interactions, in order."""
        inter = []
        launched = 0
        while launched < n_rollouts:
            actual = min(n_rollouts - launched, self.B)
            self._round_episode(self._round_seeds(actual, seed_generator), env_options, actual, **run_kw)
            self.episodes += 1
            launched += actual
            for ep in self.interactions(actual):
                inter.append(ep)
                if interaction_callback is not None:
                    interaction_callback(ep)
        return inter
