"""Lock-step chess rollouts on the device: the chess twin of `MazeRolloutEngine` for configs[3].

The MI355X counterpart of `interact_environment(FenChessHistoryEnv(...), GPT2PPOPolicy(...), bsize=B)` as the online PPO script runs it
(llm_rl_scripts/chess/ppo/train_ppo_gpt2_online.py:201-340 with chess/env/env.py:91-238).  The boards already step on the device
(csrc/chess.hip, csrc/chess_rules.h); here the text around them stays there too (csrc/chess_tokens.hip).  A turn is

    FEN bytes -> prompt ids, 16-token chunks | prefill behind the kept prefix | generate <= max_new ids | ids -> SAN bytes | agent half-step |
    opponent reply + half-step | record, next FEN

A chess prompt is `' '.join(fen)` of the current position alone (`preprocess_state_og`), so there is no history window and no prefix cache;
consecutive prompts of a game share a prefix (all of it after an illegal move), whose K/V rows are kept as the generic policy keeps them.
With the device opponent (a uniformly random legal move from a counter-based stream of this package's own, or an injected index table) nothing
leaves HBM during an episode and one turn is one hipGraph replay; with a host engine pool (Stockfish over UCI) the turn runs eagerly in two
halves around one hand-off: the agents' moves `[B][8]` go down, the replies `[B][8]` come up.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np

from . import _lib
from .envs import chess as C
from .gpt2 import FWD_RAGGED_ALWAYS
from .maze_rollout import _decode_one, maze_out_str_process, token_byte_table
from .turn_loop import TurnLoopEngine, decode_generation, summarize

FEN_BYTES, ACTION_BYTES = C.FEN_BYTES, C.ACTION_BYTES
_FIELDS = ("fen", "gen", "gen_len", "action", "result", "reward", "done", "opp_san", "reply", "n_turns", "live", "ep_reward", "cur_fen", "cur_len", "prev_fen", "prev_len", "keep", "out_tok",
           "out_len", "gen_active", "act", "res", "rew", "dn", "uci", "cur_reply", "reply_ok", "cur_san", "flags")
_PROBE_FENS = (C.START_FEN, "7k/5Q2/6K1/8/8/8/8/8 w - - 0 1", "r3k2r/pppq1ppp/2n2n2/3Pp3/8/2N2N2/PPP2PPP/R3K2R w KQkq e6 0 10",
               "8/1k6/8/8/3R4/8/5K2/8 b - - 37 112")
_FEN_ALPHABET = "pnbrqkPNBRQK/0123456789 wb-abcdefgh"


class _CTraj(ctypes.Structure):            # lmrl_chess_traj (include/lmrl_amd.h)
    _fields_ = [(n, ctypes.c_void_p) for n in _FIELDS]


def chess_token_tables(tokenizer, vocab: int):
    """(byte_id int32 [256], tok_bytes uint8 [vocab][16], tok_blen uint8 [vocab], byte_ids bool) for `lmrl_chess_tok_create`.  Raises ValueError
    when the tokenizer does not encode `' '.join(fen)` as the concatenation of its single characters' encodings, one id each (GPT-2 BPE merges
    them: use the generic text path)."""
    enc = lambda s: list(tokenizer.encode(s))
    byte_id = np.full(256, -1, dtype=np.int32)
    for c in range(128):
        try:
            ids = enc(chr(c))
        except (KeyError, ValueError):              # a character the tokenizer does not know
            continue
        if len(ids) == 1:
            byte_id[c] = ids[0]
    missing = [ch for ch in _FEN_ALPHABET if byte_id[ord(ch)] < 0]
    if missing:
        raise ValueError(f"ChessRolloutEngine: the tokenizer has no single id for {missing!r} — use E.text_env_eval(VectorChessEnv, GPT2PPOPolicy)")
    for f in _PROBE_FENS:
        text = C.preprocess_state_og(f)
        if enc(text) != [int(byte_id[ord(ch)]) for ch in text]:
            raise ValueError("ChessRolloutEngine: this tokenizer does not encode ' '.join(fen) character by character (a BPE tokenizer merges them) — "
                             "use E.text_env_eval(VectorChessEnv, GPT2PPOPolicy)")
    tb, bl = token_byte_table(tokenizer, vocab)
    # ids 0..255 = the text's UTF-8 bytes, every other id decodes to nothing?  Then generations are decoded as UTF-8 on the device.
    byte_ids = len(tokenizer) >= 256
    if byte_ids:
        probe = [C.preprocess_state_og(_PROBE_FENS[0]), "Q h 5\n", "café  x", "\U0001F600"]
        try:
            byte_ids = all(enc(x) == list(x.encode("utf-8")) for x in probe) and all(_decode_one(tokenizer, i) == chr(i) for i in range(128)) and \
                all(_decode_one(tokenizer, i) == "" for i in range(256, min(len(tokenizer), 1024))) and \
                tokenizer.decode([0xC3, 0xA9, 0xC3, 0x41, 0xE2, 0x82]) == "éA"
        except Exception:
            byte_ids = False
    return byte_id, tb, bl, bool(byte_ids)


def chess_summary(interactions):
    """The summary of `text_env_eval_chess_positions` (chess/env/env.py:257-342) over finished episodes."""
    rs, dones, victories, percent_illegals, episode_length = [], [], [], [], []
    for interaction in interactions:
        rewards = [x.reward for x in interaction]
        victories.append(1 if 1 in rewards else 0)
        num_illegal = sum(1 if x.reward == -1 and i < len(rewards) - 1 else 0 for i, x in enumerate(interaction))
        percent_illegals.append(num_illegal / len(rewards) * 100)
        episode_length.append(len(rewards))
        rs.append(sum(rewards))
        dones.append(interaction[-1].done)
    summ = summarize
    return dict(reward=summ(np.asarray(rs, dtype=np.float32)), done=summ(np.asarray(dones, dtype=np.float32)), victories=summ(victories),
                percent_illegals=summ(percent_illegals), episode_length=summ(episode_length), length=summ(episode_length))


class ChessRolloutEngine(TurnLoopEngine):
    """B lock-step chess episodes (`FenChessHistoryEnv`: the observation is the current position, `preprocess_state_og`) driven by a GPT-2 policy
    on one GPU; the public face mirrors `MazeRolloutEngine`.

    `env`: a `FenChessHistoryEnv` / `VectorChessEnv` — `max_moves`, `from_position` and `state_fn` are taken from it; only
    `state_fn = preprocess_state_og` without `initial_history` is in scope (anything else: the generic path, `E.text_env_eval(VectorChessEnv(...),
    GPT2PPOPolicy(...))`).  `opponent`: "device" (a random legal move drawn on the device — `lmrl_chess_tok_opponent`'s documented counter stream —
    or `set_scripted_replies`) or an `EnginePool`-like object with `best_moves([(start_fen, [uci, ...]), ...]) -> [uci, ...]`.
    `engine`: a `GPT2Engine` (bf16) or a `GPT2EngineF32`.  The policy's `out_str_process` is the scripts' `removesuffix('\\n') + '\\n'`.
    `prompt_bound`: an upper bound of the prompt length in tokens (default: what a FEN of LMRL_CHESS_FEN_BYTES can need, cut to
    `max_input_length`) — it fixes the number of 16-token prefill chunks per turn; `records()` raises if a prompt ever exceeded it.
    `reuse_kv` (default, as `GPT2PPOPolicy`): the K/V rows of the longest common prefix of the previous and the current prompt stay in the cache
    and only the rest is forwarded (`lmrl_chess_tok_prefix`) — one token after an illegal move, the part behind the first changed square after a
    move; False: every turn prefills from position 0."""

    def __init__(self, engine, tokenizer, env, batch: int, max_new_tokens: int = 8, eos_token_id: Optional[int] = None, max_input_length: int = 256,
                 max_turns: Optional[int] = None, opponent="device", prompt_bound: Optional[int] = None, reuse_kv: bool = True,
                 session_flags: int = FWD_RAGGED_ALWAYS):
        from .gptj_f32_engine import refuse_gptj
        refuse_gptj("ChessRolloutEngine", engine)
        import torch
        t = torch
        venv = getattr(env, "_vec", env)
        if not isinstance(venv, C.VectorChessEnv) or venv.state_fn is not C.preprocess_state_og or tuple(venv.initial_history):
            raise ValueError("ChessRolloutEngine: only FenChessHistoryEnv-style envs (state_fn = preprocess_state_og, no initial_history) run on the device "
                             "loop — use E.text_env_eval(env, GPT2PPOPolicy(...)) for anything else")
        self.max_moves, self.start = int(venv.max_moves), venv.start
        if max_turns is None:
            max_turns = self.max_moves + 1          # the move after max_moves moves ends the episode (num_moves_made > max_moves)
        self.eng, self.tok, self.env, self.B = engine, tokenizer, venv, int(batch)
        self.max_new, self.T = int(max_new_tokens), int(max_turns)
        if not 0 < self.T < 4096:
            raise ValueError("ChessRolloutEngine: max_turns must be in [1, 4095] (the reply stream's episode word keeps 12 bits for the turn)")
        self.eos = eos_token_id if eos_token_id is not None else getattr(tokenizer, "eos_token_id", None)
        self.pad = getattr(tokenizer, "pad_token_id", 0) or 0
        self.dev, self._L = engine.device, _lib.lib()
        self._max_input_length = int(max_input_length)
        self.opponent = opponent
        self.reuse_kv = bool(reuse_kv)
        if opponent != "device" and not hasattr(opponent, "best_moves"):
            raise ValueError("ChessRolloutEngine: opponent is \"device\" or an object with best_moves(games)")
        byte_id, tb, bl, self._byte_ids = chess_token_tables(tokenizer, engine.cfg.vocab)
        self._tok = self._L.lmrl_chess_tok_create(byte_id.ctypes.data, tb.ctypes.data, bl.ctypes.data, engine.cfg.vocab, 1 if self._byte_ids else 0,
                                                  -1 if self.eos is None else int(self.eos), self.max_new, self.T, 0)
        if not self._tok:
            raise _lib.LmrlError(self._L.lmrl_last_error().decode())
        full = min(2 * (FEN_BYTES - 1) - 1, self._max_input_length)
        self.prompt_bound = full if prompt_bound is None else min(int(prompt_bound), full)
        self.n_chunks = -(-self.prompt_bound // 16)
        tmax = self.n_chunks * 16 + -(-self.max_new // 16) * 16
        self.ses = engine.session(self.B, tmax, flags=session_flags)
        B, G, T = self.B, self.max_new, self.T
        z = lambda *shape, dt: t.zeros(*shape, dtype=dt, device=self.dev)
        u8, i32, f32 = t.uint8, t.int32, t.float32
        self.traj = dict(fen=z(B, T, FEN_BYTES, dt=u8), gen=z(B, T, G, dt=i32), gen_len=z(B, T, dt=i32), action=z(B, T, ACTION_BYTES, dt=u8),
                         result=z(B, T, dt=u8), reward=z(B, T, dt=f32), done=z(B, T, dt=u8), opp_san=z(B, T, ACTION_BYTES, dt=u8), reply=z(B, T, 8, dt=u8),
                         n_turns=z(B, dt=i32), live=z(B, dt=u8), ep_reward=z(B, dt=f32), cur_fen=z(B, FEN_BYTES, dt=u8), cur_len=z(B, dt=i32),
                         prev_fen=z(B, FEN_BYTES, dt=u8), prev_len=z(B, dt=i32), keep=z(B, dt=i32),
                         out_tok=z(B, G, dt=i32), out_len=z(B, dt=i32), gen_active=z(B, dt=u8), act=z(B, ACTION_BYTES, dt=u8), res=z(B, dt=u8),
                         rew=z(B, dt=f32), dn=z(B, dt=u8), uci=z(B, 8, dt=u8), cur_reply=z(B, 8, dt=u8), reply_ok=z(B, dt=u8),
                         cur_san=z(B, ACTION_BYTES, dt=u8), flags=z(1, dt=i32))
        self._ctraj = _CTraj(*[self.traj[n].data_ptr() for n in _FIELDS])
        self.pos = z(B * self._L.lmrl_chess_pos_bytes(), dt=u8)
        self.fens_d, self.ok = z(B, FEN_BYTES, dt=u8), z(B, dt=u8)
        self._alloc_turn_loop()              # (`epoch` is the 4th counter word of the reply stream too)
        self.turn_graph = None
        self._replies = None                 # int32 [T][B] injected reply indices
        self._starts: List[str] = [self.start] * B
        self._moves: List[List[str]] = [[] for _ in range(B)]

    def close(self):
        if getattr(self, "_tok", None):
            self._L.lmrl_chess_tok_destroy(self._tok)
            self._tok = None

    # ---- scripted workloads ------------------------------------------------------------------------------------------------------------
    def set_scripted_actions(self, san_strings, strength: float = 30.0, spaced: bool = True) -> None:
        """Synthetic-workload hook (tools, tests; as `MazeRolloutEngine.set_scripted_actions`): `san_strings` [T][B] of str (None: no steering) — in
        turn t the sampler of env b is steered (+`strength` on one logit per generated position; every logit is still computed and sampled) towards
        spelling that string the way the chess data spells moves (`preprocess_move`: blanks between the characters, a newline; `spaced=False`: the
        bare string and a newline), cut to max_new_tokens ids.  None switches it off.  Captured turn graphs are dropped."""
        self.turn_graph = None
        if san_strings is not None:
            assert len(san_strings) == self.T and all(len(r) == self.B for r in san_strings)
            spell = lambda s: None if s is None else self.tok.encode(C.preprocess_move(s) if spaced else s + "\n")
            san_strings = [[spell(s) for s in row] for row in san_strings]
        self._set_script(san_strings, strength)

    def set_scripted_replies(self, idx) -> None:
        """Device opponent: in turn t game b is answered with legal move `idx[t][b] mod count` in `lmrl_chess_describe`'s order instead of a drawn
        one.  None: back to the reply stream.  Captured turn graphs are dropped."""
        import torch
        self.turn_graph = None
        if idx is None:
            self._replies = None
            return
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        assert idx.ndim == 2 and idx.shape[1] == self.B and idx.shape[0] >= 1
        self._replies = torch.from_numpy(idx).to(self.dev)

    # ---- weights -----------------------------------------------------------------------------------------------------------------------
    def set_params(self, engine) -> None:
        """Swap in freshly trained policy weights (PPOPolicy.set_params, ppo/base_interface.py:821-823)."""
        self.eng = engine
        self.ses = engine.session(self.B, self.ses.tmax, flags=self.ses.flags)
        self.turn_graph = None

    # ---- one lock-step turn ------------------------------------------------------------------------------------------------------------
    def _agent_half(self, temperature: float, top_k: int, sample_seed: int, logits_out=None):
        """The kept prompt prefix, the prompt chunks behind it, the decode steps, ids -> SAN -> the agent's half-step."""
        L, sp, tr, B = self._L, _lib.stream_ptr(), ctypes.byref(self._ctraj), self.B
        ck = _lib.check
        self.ses.reset()
        ck(L.lmrl_chess_tok_prefix(self._tok, tr, self._max_input_length, 1 if self.reuse_kv else 0, _lib.ptr(self.ses.len), B, sp), "lmrl_chess_tok_prefix")
        for j in range(self.n_chunks):
            ck(L.lmrl_chess_tok_prompt(self._tok, tr, j, 16, self._max_input_length, self.n_chunks, _lib.ptr(self.chunk_tok), _lib.ptr(self.chunk_cnt), B, sp),
               "lmrl_chess_tok_prompt")
            self.ses.forward(self.chunk_tok, self.chunk_cnt, 16, len_bound_after=self.n_chunks * 16)
        g = self.traj
        self._generate(self.ses, (self.ses,), temperature, top_k, 0.0, sample_seed, 0.0, _lib.ptr(self.epoch), g["gen_active"], g["out_tok"], g["out_len"],
                       self.next_tok, self.next_cnt, -1 if self.eos is None else int(self.eos), self.max_new, self._steer_rows(), logits_out)
        ck(L.lmrl_chess_tok_action(self._tok, tr, _lib.ptr(self.pos), B, sp), "lmrl_chess_tok_action")

    def _finish(self):
        L, sp, tr = self._L, _lib.stream_ptr(), ctypes.byref(self._ctraj)
        _lib.check(L.lmrl_chess_tok_result(self._tok, tr, _lib.ptr(self.pos), self.max_moves, self.B, sp), "lmrl_chess_tok_result")
        self._end_turn(self._script)

    def _turn(self, temperature: float, top_k: int, sample_seed: int, logits_out=None):
        """Device opponent: the whole turn, no host round trip (graph-capturable)."""
        L, sp, tr = self._L, _lib.stream_ptr(), ctypes.byref(self._ctraj)
        self._agent_half(temperature, top_k, sample_seed, logits_out)
        rp = self._replies
        _lib.check(L.lmrl_chess_tok_opponent(self._tok, tr, _lib.ptr(self.pos), int(sample_seed) & (2 ** 64 - 1), _lib.ptr(self.epoch), _lib.ptr(rp),
                                             int(rp.shape[0]) if rp is not None else 0, self.B, sp), "lmrl_chess_tok_opponent")
        self._finish()

    def _turn_host(self, temperature: float, top_k: int, sample_seed: int, logits_out=None):
        """Host engine pool: two halves around one hand-off — the agents' moves [B][8] down, the replies [B][8] up."""
        import torch
        L, sp, tr = self._L, _lib.stream_ptr(), ctypes.byref(self._ctraj)
        self._agent_half(temperature, top_k, sample_seed, logits_out)
        played = C.VectorChessBoards._unpack(self.traj["uci"].view(-1), 8)
        idx = [b for b, mv in enumerate(played) if mv]
        if idx:
            for b in idx:
                self._moves[b].append(played[b])
            replies = self.opponent.best_moves([(self._starts[b], self._moves[b]) for b in idx])
            up = np.zeros((self.B, 8), dtype=np.uint8)
            for b, mv in zip(idx, replies):
                raw = mv.encode("ascii", errors="replace")[:7]
                up[b, : len(raw)] = np.frombuffer(raw, dtype=np.uint8)
                self._moves[b].append(mv)
            self.traj["cur_reply"].copy_(torch.from_numpy(up))
            _lib.check(L.lmrl_chess_tok_opponent_host(self._tok, tr, _lib.ptr(self.pos), self.B, sp), "lmrl_chess_tok_opponent_host")
            ok = self.traj["reply_ok"].cpu().numpy()
            for b, mv in zip(idx, replies):
                if not ok[b]:
                    raise RuntimeError(f"engine move {mv!r} is not legal in game {b}")
        self._finish()

    def capture_turn(self, temperature: float = 1.0, top_k: int = 0, sample_seed: int = 0):
        """One turn (device opponent) as a hipGraph; `run_episode(..., use_graph=True)` replays it per turn."""
        if self.opponent != "device":
            raise _lib.LmrlError("ChessRolloutEngine.capture_turn: a turn with a host engine pool has a host hand-off in the middle — it runs eagerly")
        self._begin_capture(temperature, top_k, 0.0, sample_seed)
        self._begin([self.start] * self.B)
        self.turn_graph = self._capture(temperature, top_k, sample_seed, self._logits)
        return self.turn_graph

    def _graphs(self):
        return self.turn_graph

    def _recapture(self, temperature, top_k, top_p, sample_seed):
        self.capture_turn(temperature, top_k, sample_seed)

    def _begin(self, starts: List[str], n_live: Optional[int] = None):
        import torch
        buf = np.zeros((self.B, FEN_BYTES), dtype=np.uint8)
        for i, s in enumerate(starts):
            raw = s.encode("ascii", errors="replace")[: FEN_BYTES - 1]
            buf[i, : len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        self.fens_d.copy_(torch.from_numpy(buf))
        _lib.check(self._L.lmrl_chess_tok_begin(self._tok, ctypes.byref(self._ctraj), _lib.ptr(self.pos), _lib.ptr(self.fens_d), _lib.ptr(self.ok), self.B,
                                                _lib.stream_ptr()), "lmrl_chess_tok_begin")
        if n_live is not None and n_live < self.B:       # the idle envs of a partial last batch
            self.traj["live"][n_live:] = 0
            self.traj["gen_active"][n_live:] = 0
        self._starts, self._moves = list(starts), [[] for _ in range(self.B)]

    def _episode_begin(self, seeds, options, temperature, top_k, sample_seed, episode, use_graph, n_live=None):
        logits = self._episode_logits(use_graph, temperature, top_k, 0.0, sample_seed)
        assert len(seeds) == self.B
        if options is not None and not isinstance(options, (list, tuple)):
            options = [options] * self.B
        starts = [(o or {}).get("from_position", self.start) for o in options] if options is not None else [self.start] * self.B
        self._begin(starts, n_live)
        bad = np.nonzero(self.ok.cpu().numpy() == 0)[0]
        if len(bad):
            raise ValueError(f"invalid FEN: {starts[int(bad[0])]!r}")
        self._start_episode_counters(episode)
        if use_graph:
            return self.turn_graph.replay
        fn = self._turn if self.opponent == "device" else self._turn_host
        return lambda: fn(temperature, top_k, sample_seed, logits)

    def run_episode(self, seeds, options=None, temperature: float = 1.0, top_k: int = 0, sample_seed: int = 0, episode: int = 0, use_graph: bool = False,
                    sync_every: int = 8, max_turns: Optional[int] = None, n_live: Optional[int] = None):
        """One full episode for all B games; returns the device record dict (read after a sync).  `seeds` are accepted for the common face (the
        chess env's reset ignores them); `options`: one dict or one per env, `{"from_position": fen}` as `VectorChessEnv.reset`.  The host peeks at
        the live flags every `sync_every` turns to stop early (0: never)."""
        if use_graph and self.opponent != "device":
            raise _lib.LmrlError("ChessRolloutEngine: use_graph needs the device opponent")
        turn = self._episode_begin(seeds, options, temperature, top_k, sample_seed, episode, use_graph, n_live)
        return self._run_turns(lambda i: turn(), sync_every, max_turns)

    # ---- host views --------------------------------------------------------------------------------------------------------------------
    def _check_flags(self):
        if int(self.traj["flags"].cpu().numpy()[0]) & 1:
            raise _lib.LmrlError(f"ChessRolloutEngine: a prompt was longer than prompt_bound = {self.prompt_bound} tokens — the episode fed cut prompts")

    @staticmethod
    def _cut(row) -> str:
        return row.tobytes().split(b"\0")[0].decode("ascii", errors="replace")

    def records(self):
        """Host copies per game: dict(fen [n] position texts, gen id lists, action SAN strings, result uint8 [n], reward f32 [n], done bool [n],
        opp_san / reply [n] ('' where there was no reply), final_fen, live)."""
        self._check_flags()
        h = {k: v.cpu().numpy() for k, v in self.traj.items()}
        out = []
        for b in range(self.B):
            n = int(h["n_turns"][b])
            out.append(dict(fen=[self._cut(h["fen"][b, i]) for i in range(n)], gen=[h["gen"][b, i, : h["gen_len"][b, i]].tolist() for i in range(n)],
                            action=[self._cut(h["action"][b, i]) for i in range(n)], result=h["result"][b, :n].copy(), reward=h["reward"][b, :n].copy(),
                            done=h["done"][b, :n].astype(bool), opp_san=[self._cut(h["opp_san"][b, i]) for i in range(n)],
                            reply=[self._cut(h["reply"][b, i]) for i in range(n)], final_fen=self._cut(h["cur_fen"][b]), live=bool(h["live"][b]),
                            ep_reward=float(h["ep_reward"][b])))
        return out

    def interactions(self, n: Optional[int] = None):
        """The finished episodes (of the first `n` games) as `List[List[InteractionTransition]]` — what `interact_environment` returns for the same
        rollouts (LLM_RL/environment.py:154-207 on FenChessHistoryEnv)."""
        from .environment import InteractionTransition, Text
        out = []
        for rec in self.records()[: self.B if n is None else int(n)]:
            obs = [(Text(C.preprocess_state_og(f), False),) for f in rec["fen"] + [rec["final_fen"]]]
            trans = []
            for i in range(len(rec["fen"])):
                act = Text(maze_out_str_process(decode_generation(self.tok, rec["gen"][i], self.eos)), True)
                trans.append(InteractionTransition(obs[i], obs[i] + (act,), obs[i + 1], float(rec["reward"][i]), bool(rec["done"][i])))
            out.append(trans)
        return out

    def text_env_eval(self, n_rollouts: int, seed_generator=None, env_options=None, temperature: float = 1.0, top_k: int = 0, sample_seed: int = 0,
                      interaction_callback=None, use_graph: Optional[bool] = None, sync_every: int = 8):
        """`text_env_eval(env, policy, n_rollouts, bsize=B, env_options=...)` with the lock-step loop on the device: ceil(n / B) episode batches, the
        (interactions, summary) of `text_env_eval_chess_positions` for this env's start position — reward / done / victories / percent_illegals /
        episode_length (+ `length`, E.text_env_eval's name for the last).  The sampler's and the reply stream's episode word keeps counting across
        calls.  `use_graph` defaults to the device opponent's graph path."""
        if use_graph is None:
            use_graph = self.opponent == "device"
        inter = self._eval_round(n_rollouts, seed_generator, env_options, interaction_callback,
                                 dict(temperature=temperature, top_k=top_k, sample_seed=sample_seed, use_graph=use_graph, sync_every=sync_every))
        return inter, chess_summary(inter)

    # ---- the online-RL hand-over -------------------------------------------------------------------------------------------------------
    def ppo_records(self, n: Optional[int] = None):
        """The finished episodes (of the first `n` games; default all) as `algorithms.ppo_device.PPORecords`: one token trajectory per transition
        (the observation's prompt ids ++ the action ids, the reward on the action's last token), chained per episode — the chains the online script
        builds from `raw_results` (chess/ppo/train_ppo_gpt2_online.py:293-314) after `TokenTrajectory.from_text_trajectory`.  The observation ids are
        the full prompt (the chains tokenise the text itself, whatever `max_input_length` cut for the policy); the action ids re-encode the action
        text (`lmrl_chess_tok_ppo_records`)."""
        import torch
        from .algorithms.ppo_device import PPORecords
        t, L, sp = torch, self._L, _lib.stream_ptr()
        self._check_flags()
        B = self.B if n is None else int(n)
        off = t.empty(B + 1, dtype=t.int32, device=self.dev)
        _lib.check(L.lmrl_exclusive_scan_i32(_lib.ptr(self.traj["n_turns"]), _lib.ptr(off), B, sp), "lmrl_exclusive_scan_i32")
        N = int(off[B:].cpu().numpy()[0])
        if N == 0:
            raise ValueError("ppo_records: no transition recorded (run an episode first)")
        nl = self.tok.encode("\n")
        assert len(nl) == 1, "the newline must be one token"
        cap = 2 * (FEN_BYTES - 1) - 1 + self.max_new + 1
        z = lambda *s_, dt: t.zeros(*s_, dtype=dt, device=self.dev)
        tokens, ia, rw = z(N, cap, dt=t.int32), z(N, cap, dt=t.uint8), z(N, cap, dt=t.float32)
        n_tok, chain, pos, last = z(N, dt=t.int32), z(N, dt=t.int32), z(N, dt=t.int32), z(N, dt=t.uint8)
        done, total = z(B, dt=t.uint8), z(B, dt=t.int32)
        _lib.check(L.lmrl_chess_tok_ppo_records(self._tok, ctypes.byref(self._ctraj), B, _lib.ptr(off), int(nl[0]), cap, _lib.ptr(tokens), _lib.ptr(ia),
                                                _lib.ptr(rw), _lib.ptr(n_tok), _lib.ptr(chain), _lib.ptr(pos), _lib.ptr(last), _lib.ptr(done), _lib.ptr(total), sp),
                   "lmrl_chess_tok_ppo_records")
        return PPORecords(tokens, ia, rw, n_tok, done, chain, pos, last, n_chains=B, chain_len_bound=max(int(total.cpu().numpy().max()), 1))

    def ppo_rollouts(self, inference, n_rollouts: int, seed_generator=None, env_options=None, *, gamma: float, lam: float, kl_weight: float,
                     max_length: Optional[int] = None, use_advantage_whitening: bool = True, temperature: float = 1.0, top_k: int = 0, sample_seed: int = 0,
                     use_graph: Optional[bool] = None, **kw):
        """One data-collection round of the online PPO loop on the device: `text_env_eval(n_rollouts, bsize=B)` + `ppo_dataset_loader` ->
        (DevicePPODataset over all transitions of all rollouts, all_kls, summary).  Per episode batch: the lock-step episode, then its PPO data while
        the record is in the engine's buffers; advantages whitened once over the action tokens of the whole round; `summary` has `text_env_eval`'s
        fields (from the record's rewards; no text is built)."""
        if use_graph is None:
            use_graph = self.opponent == "device"
        return self._ppo_round(inference, n_rollouts, seed_generator, env_options, use_advantage_whitening,
                               dict(temperature=temperature, top_k=top_k, sample_seed=sample_seed, use_graph=use_graph),
                               dict(gamma=gamma, lam=lam, kl_weight=kl_weight, max_length=max_length, **kw))

    _DRAW_SEEDS = False          # the chess env's reset ignores its seeds
    _SUMMARY = (("reward", 0, np.float32), ("done", 1, np.float32), ("victories", 2, np.float64), ("percent_illegals", 3, np.float64),
                ("episode_length", 4, np.int64), ("length", 4, np.int64))

    def _round_stats(self, actual: int):
        rw = self.traj["reward"][:actual].cpu().numpy(); dn = self.traj["done"][:actual].cpu().numpy(); nt = self.traj["n_turns"][:actual].cpu().numpy()
        stats = []
        for b in range(actual):
            r = rw[b, : nt[b]]
            stats.append((float(r.sum()), float(dn[b, max(nt[b] - 1, 0)]), float(1 in r), float((r[:-1] == -1).sum()) / max(len(r), 1) * 100, int(nt[b])))
        return np.asarray(stats, dtype=np.float64).T
