"""Lock-step Twenty Questions rollouts on the device: the twin of `ChessRolloutEngine` / `MazeRolloutEngine` for the env with TWO models in the loop.

The MI355X counterpart of `interact_environment(BatchedTwentyQuestionsPolicyEnvironment(GPT2EngineOracle(...)), GPT2PPOPolicy(...), bsize=B)` as
the PPO script runs it (llm_rl_scripts/twenty_questions/ppo/train_ppo.py:312-352 with twenty_questions/env/{env,data,oracle}.py).  The generic path
decodes the question, builds B oracle prompt strings, tokenises them, runs the oracle policy, regex-parses B answers, runs `is_done` in Python and
hands text back to the guesser, which tokenises the whole history again — every turn.  Here the text stays in HBM (csrc/tq_tokens.hip, the rules:
csrc/tq_core.h) and a turn is

    guesser decode | question: ids -> text -> canonical ids, strip, oracle prompt | oracle prefill behind its kept prefix | <= 4 greedy steps |
    answer: ids -> "Yes." / "No." | judge: guessed, reward, done, record | guesser chunk: the question's unforwarded tail + the answer

on two sessions — the guesser's persistent per-env KV cache, which only ever grows (the history is never truncated in scope), and the oracle's,
whose prompt prefix "Answer the question ... object: {word}\\nquestion: " survives from turn to turn by the generic policy's own rule (the longest
common prefix of consecutive prompts).  One turn is one hipGraph replay (two captured kinds: an episode's first turn prefills the whole oracle
prompt, later turns only the part behind the kept prefix).
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional

import numpy as np

from . import _lib
from .envs import twenty_questions as TQ
from .gpt2 import FWD_RAGGED_ALWAYS
from .maze_rollout import _decode_one, maze_out_str_process, token_byte_table
from .turn_loop import TurnLoopEngine, decode_generation, summarize

ORACLE_PREFIX = "Answer the question about the object truthfully.\nobject: {word}\nquestion: "
ORACLE_SUFFIX = "\nanswer (yes or no): "
_FIELDS = ("gen", "gen_len", "q_text", "q_len", "q_off", "ogen", "ogen_len", "answer", "reward", "done", "flag", "n_turns", "live", "ep_reward", "word",
           "out_tok", "out_len", "gen_active", "o_out_tok", "o_out_len", "o_active", "strip_b", "strip_e", "ans", "hist", "hist_len", "feed_start", "feed_len",
           "o_prompt", "o_len", "o_prev", "o_prev_len", "o_keep", "flags")
_GENERIC = "use E.text_env_eval(env, GPT2PPOPolicy(...)), the generic text path"


class _CTraj(ctypes.Structure):            # lmrl_tq_traj (include/lmrl_amd.h)
    _fields_ = [(n, ctypes.c_void_p) for n in _FIELDS] + [("hcap", ctypes.c_int32), ("pcap", ctypes.c_int32)]


class _CTables(ctypes.Structure):          # lmrl_tq_tables (include/lmrl_amd.h)
    _fields_ = [("bytes", ctypes.c_void_p), ("str_off", ctypes.c_void_p), ("spell_off", ctypes.c_void_p), ("word_off", ctypes.c_void_p),
                ("n_strings", ctypes.c_int32), ("n_spellings", ctypes.c_int32), ("n_words", ctypes.c_int32), ("n_det", ctypes.c_int32),
                ("n_func", ctypes.c_int32), ("n_generic", ctypes.c_int32), ("tok_blen", ctypes.c_void_p), ("vocab", ctypes.c_int32),
                ("eos_token", ctypes.c_int32), ("oracle_eos_token", ctypes.c_int32), ("prefix", ctypes.c_void_p), ("prefix_len", ctypes.c_void_p),
                ("prefix_cap", ctypes.c_int32), ("suffix", ctypes.c_void_p), ("suffix_len", ctypes.c_int32), ("invalid_question", ctypes.c_void_p),
                ("invalid_len", ctypes.c_int32), ("initial", ctypes.c_void_p), ("initial_len", ctypes.c_int32), ("yes", ctypes.c_void_p),
                ("yes_len", ctypes.c_int32), ("no", ctypes.c_void_p), ("no_len", ctypes.c_int32), ("max_new_tokens", ctypes.c_int32),
                ("oracle_max_new_tokens", ctypes.c_int32), ("max_turns", ctypes.c_int32)]


def ids_are_utf8_bytes(tokenizer, probes) -> bool:
    """Are this tokenizer's ids 0..255 the text's UTF-8 bytes, every other id decoding to nothing, invalid sequences dropped (the probe of
    `chess_token_tables`, on this env's own strings)?"""
    if len(tokenizer) < 256:
        return False
    try:
        return all(list(tokenizer.encode(x)) == list(x.encode("utf-8")) for x in list(probes) + ["café  x", "\U0001F600", "　a\x85"]) and \
            all(_decode_one(tokenizer, i) == chr(i) for i in range(128)) and \
            all(_decode_one(tokenizer, i) == "" for i in range(256, min(len(tokenizer), 1024))) and \
            tokenizer.decode([0xC3, 0xA9, 0xC3, 0x41, 0xE2, 0x82]) == "éA"
    except Exception:
        return False


def tq_context(tokenizer, vocab: int, word_list, max_new_tokens: int, max_turns: int, eos_token_id: Optional[int], oracle_max_new_tokens: int = 4,
               host_only: bool = False):
    """`lmrl_tq_create` on the tables of this word list and tokenizer -> (context handle, info dict: prefix_cap / suffix_len / invalid_len /
    initial_len / answer_len).  Raises ValueError for a tokenizer whose ids are not the text's UTF-8 bytes."""
    words = list(word_list)
    if not words:
        raise ValueError("TwentyQuestionsRolloutEngine: empty word list")
    prefixes = [ORACLE_PREFIX.format(word=w) for w in words]
    assert TQ.get_oracle_prompt(words[0], "q") == prefixes[0] + "q" + ORACLE_SUFFIX, "the oracle prompt's layout changed"
    if not ids_are_utf8_bytes(tokenizer, [TQ.INITIAL_STR, TQ.INVALID_QUESTION, prefixes[0], ORACLE_SUFFIX, "Yes.\n", "No.\n", "Is it an animal?\n"]):
        raise ValueError("TwentyQuestionsRolloutEngine: this tokenizer's ids are not the text's UTF-8 bytes (a merging tokenizer encodes the history, "
                         f"the questions and the oracle prompts differently) — {_GENERIC}")
    enc = lambda s: np.asarray(list(tokenizer.encode(s)), dtype=np.int32)
    strings: List[bytes] = [s.encode("utf-8") for s in sorted(TQ._DETERMINERS)] + [s.encode("utf-8") for s in sorted(TQ._FUNCTION_WORDS)] + \
        [s.encode("utf-8") for s in sorted(TQ._GENERIC_NOUNS)]
    n_fixed = len(strings)
    spell_off, word_off = [n_fixed], [0]
    for w in words:
        for sp in w.tokens:
            strings.extend(t.encode("utf-8") for t in sp)
            spell_off.append(len(strings))
        word_off.append(len(spell_off) - 1)
    blob = np.frombuffer(b"".join(strings) or b"\0", dtype=np.uint8).copy()
    str_off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int32)
    spell_off, word_off = np.asarray(spell_off, dtype=np.int32), np.asarray(word_off, dtype=np.int32)
    pre = [enc(p) for p in prefixes]
    prefix_cap = max(len(p) for p in pre)
    prefix = np.zeros((len(words), prefix_cap), dtype=np.int32)
    for i, p in enumerate(pre):
        prefix[i, : len(p)] = p
    prefix_len = np.asarray([len(p) for p in pre], dtype=np.int32)
    suffix, initial, yes, no = enc(ORACLE_SUFFIX), enc(TQ.INITIAL_STR), enc("Yes.\n"), enc("No.\n")
    invalid = np.frombuffer(TQ.INVALID_QUESTION.encode("utf-8"), dtype=np.uint8).copy()
    _, tok_blen = token_byte_table(tokenizer, vocab)
    nl = list(tokenizer.encode("\n"))
    assert len(nl) == 1, "the newline must be one token"
    p = lambda a: a.ctypes.data
    tab = _CTables(p(blob), p(str_off), p(spell_off), p(word_off), len(strings), len(spell_off) - 1, len(words), len(TQ._DETERMINERS), len(TQ._FUNCTION_WORDS),
                   len(TQ._GENERIC_NOUNS), p(tok_blen), int(vocab), -1 if eos_token_id is None else int(eos_token_id), int(nl[0]), p(prefix), p(prefix_len),
                   prefix_cap, p(suffix), len(suffix), p(invalid), len(invalid), p(initial), len(initial), p(yes), len(yes), p(no), len(no), int(max_new_tokens),
                   int(oracle_max_new_tokens), int(max_turns))
    L = _lib.lib()
    ctx = L.lmrl_tq_create(ctypes.byref(tab), 1 if host_only else 0)
    if not ctx:
        raise _lib.LmrlError(L.lmrl_last_error().decode())
    return ctx, dict(prefix_cap=prefix_cap, suffix_len=len(suffix), invalid_len=len(invalid), initial_len=len(initial), answer_len=max(len(yes), len(no)),
                     oracle_eos=int(nl[0]))


def _is_script_out_str_process(fn: Callable[[str], str]) -> bool:
    probes = ["is it a dog", "Is it a dog?\n", "x\n\n", "", "\n", " is it.  ", "a b c d?", "what"]
    try:
        return all(fn(x) == maze_out_str_process(x) for x in probes)
    except Exception:
        return False


class TwentyQuestionsRolloutEngine(TurnLoopEngine):
    """B lock-step Twenty Questions episodes: `engine` asks, `oracle_engine` answers, on one GPU; the public face mirrors `ChessRolloutEngine`.

    `env`: a `TwentyQuestionsPolicyEnvironment` / `BatchedTwentyQuestionsPolicyEnvironment` — its `word_list` and `max_conversation_length` are
    taken (its oracle object is not used: the oracle here is `oracle_engine`, the model a `GPT2EngineOracle` would wrap).  The two engines are of
    one class and one matmul mode (bf16 `GPT2Engine`, or `GPT2EngineF32` in either mode).  The guesser's `out_str_process` is the PPO script's
    `removesuffix('\\n') + '\\n'`; the oracle generates greedily, eos = the newline id.  In scope: tokenizers whose ids are the text's UTF-8 bytes,
    conversations that fit `max_input_length` without truncation, oracle prompts that fit `oracle_max_input_length`; anything else raises
    ValueError here and stays on the generic path (so does the `asker_postproc*` family: those rewrite the question text).

    `judge`: "device" — `is_done` under the stand-in tagger `rule_pos_tag` runs in `lmrl_tq_judge`; "host" — no affirmed question is judged on the
    device; "auto" — "device" iff `rule_pos_tag` is the active tagger (and tagged the word list).  Either way an affirmed question the device did
    not judge (any code point >= 0x80; "host": every one) leaves the game running, flagged, and is re-judged after the episode with the active
    tagger through `envs.twenty_questions.is_done`: where the host says guessed the episode is cut at that turn (reward 0, done, later turns
    dropped).  Exact, because the device never ended a game the host would have continued.
    `reuse_generated` (default): the K/V rows of the generated ids stay in the guesser's cache as far as they are the question's canonical ids and
    only the rest goes through the model again; False re-forwards every question from its canonical ids, as the generic policy's prefill does."""

    def __init__(self, engine, oracle_engine, tokenizer, env, batch: int, max_new_tokens: int, eos_token_id: Optional[int], max_input_length: int,
                 oracle_max_input_length: int, oracle_max_new_tokens: int = 4, judge: str = "auto", out_str_process: Optional[Callable[[str], str]] = None,
                 reuse_generated: bool = True):
        from .gptj_f32_engine import refuse_gptj
        refuse_gptj("TwentyQuestionsRolloutEngine", engine, oracle_engine)
        import torch
        t = torch
        if not hasattr(env, "word_list") or not hasattr(env, "max_conversation_length"):
            raise ValueError(f"TwentyQuestionsRolloutEngine: env must be a Twenty Questions policy environment — {_GENERIC}")
        if type(engine) is not type(oracle_engine) or getattr(engine, "matmul", None) != getattr(oracle_engine, "matmul", None):
            raise ValueError("TwentyQuestionsRolloutEngine: the guesser's and the oracle's engine must be of one class and one matmul mode")
        if out_str_process is not None and not _is_script_out_str_process(out_str_process):
            raise ValueError("TwentyQuestionsRolloutEngine: only the PPO script's out_str_process (removesuffix('\\n') + '\\n') runs on the device loop; the "
                             f"asker_postproc family rewrites the question text — {_GENERIC}")
        if judge not in ("auto", "device", "host"):
            raise ValueError("TwentyQuestionsRolloutEngine: judge is \"auto\", \"device\" or \"host\"")
        self.eng, self.oeng, self.tok, self.env, self.B = engine, oracle_engine, tokenizer, env, int(batch)
        self.word_list = env.word_list
        self.max_new, self.omax_new, self.T = int(max_new_tokens), int(oracle_max_new_tokens), int(env.max_conversation_length)
        if not 0 < self.T < 4096 or self.max_new <= 0 or not 0 < self.omax_new <= 16:
            raise ValueError("TwentyQuestionsRolloutEngine: max_conversation_length in [1, 4095], max_new_tokens > 0, oracle_max_new_tokens in [1, 16]")
        self.eos = eos_token_id if eos_token_id is not None else getattr(tokenizer, "eos_token_id", None)
        self.pad = getattr(tokenizer, "pad_token_id", 0) or 0
        self.dev, self._L = engine.device, _lib.lib()
        self._max_input_length, self._omax_input_length = int(max_input_length), int(oracle_max_input_length)
        self.reuse_generated = bool(reuse_generated)
        TQ.pos_tag("a")                                   # resolves the default tagger
        rule = TQ._pos_tagger is TQ.rule_pos_tag and all(w.tokens == tuple(tuple(tk for tk, _ in TQ.rule_pos_tag(s.lower())) for s in w.words)
                                                           for w in self.word_list)
        if judge == "device" and not rule:
            raise ValueError("TwentyQuestionsRolloutEngine: judge=\"device\" implements the stand-in tagger rule_pos_tag only, which is not the active "
                             "tagger of this word list (judge=\"host\" re-judges affirmed questions with the active one)")
        self.judge = "device" if (judge == "device" or (judge == "auto" and rule)) else "host"
        self._tq, info = tq_context(tokenizer, engine.cfg.vocab, self.word_list, self.max_new, self.T, self.eos, self.omax_new)
        self._oeos, self._alen, self._init_len = info["oracle_eos"], info["answer_len"], info["initial_len"]
        # ---- fit without truncation
        Q = self.max_new + 1
        self.hist_bound = self._init_len + self.T * (Q + self._alen)
        if self.hist_bound > self._max_input_length or self.hist_bound + self.max_new > engine.cfg.n_pos:
            self.close()
            raise ValueError(f"TwentyQuestionsRolloutEngine: a conversation of {self.T} questions of {self.max_new} tokens can need {self.hist_bound} tokens — "
                             f"more than max_input_length = {self._max_input_length} (or the model's {engine.cfg.n_pos} positions): the history would be "
                             f"left-truncated — {_GENERIC}")
        need = info["prefix_cap"] + self.max_new + info["suffix_len"]
        self.pcap = info["prefix_cap"] + max(self.max_new, info["invalid_len"]) + info["suffix_len"]
        if need > self._omax_input_length or self.pcap + self.omax_new > oracle_engine.cfg.n_pos:
            self.close()
            raise ValueError(f"TwentyQuestionsRolloutEngine: an oracle prompt can need {need} tokens — more than oracle_max_input_length = "
                             f"{self._omax_input_length} (or the oracle's {oracle_engine.cfg.n_pos} positions) — {_GENERIC}")
        self._o_chunks = (-(-self.pcap // 16), -(-(max(self.max_new, info["invalid_len"]) + info["suffix_len"]) // 16))     # first turn, later turns
        self._g_chunks, self._init_chunks = -(-(Q + self._alen) // 16), -(-self._init_len // 16)
        # the sessions hold what the device lengths can ever reach — the whole history + one generation, the longest oracle prompt + its answer — so
        # the turns may drop the sessions' host-side overflow bound (`_len_bound = 0` in `_turn`); envs of a batch end at different turns: ragged rows
        self.ses = engine.session(self.B, -(-(self.hist_bound + self.max_new) // 16) * 16 + 16, flags=FWD_RAGGED_ALWAYS)
        self.oses = oracle_engine.session(self.B, -(-(self.pcap + self.omax_new) // 16) * 16 + 16, flags=FWD_RAGGED_ALWAYS)
        B, G, T, OG = self.B, self.max_new, self.T, self.omax_new
        z = lambda *shape, dt: t.zeros(*shape, dtype=dt, device=self.dev)
        u8, i32, f32 = t.uint8, t.int32, t.float32
        self.traj = dict(gen=z(B, T, G, dt=i32), gen_len=z(B, T, dt=i32), q_text=z(B, T, Q, dt=u8), q_len=z(B, T, dt=i32), q_off=z(B, T, dt=i32),
                         ogen=z(B, T, OG, dt=i32), ogen_len=z(B, T, dt=i32), answer=z(B, T, dt=u8), reward=z(B, T, dt=f32), done=z(B, T, dt=u8),
                         flag=z(B, T, dt=u8), n_turns=z(B, dt=i32), live=z(B, dt=u8), ep_reward=z(B, dt=f32), word=z(B, dt=i32), out_tok=z(B, G, dt=i32),
                         out_len=z(B, dt=i32), gen_active=z(B, dt=u8), o_out_tok=z(B, OG, dt=i32), o_out_len=z(B, dt=i32), o_active=z(B, dt=u8),
                         strip_b=z(B, dt=i32), strip_e=z(B, dt=i32), ans=z(B, dt=u8), hist=z(B, self.hist_bound, dt=i32), hist_len=z(B, dt=i32),
                         feed_start=z(B, dt=i32), feed_len=z(B, dt=i32), o_prompt=z(B, self.pcap, dt=i32), o_len=z(B, dt=i32), o_prev=z(B, self.pcap, dt=i32),
                         o_prev_len=z(B, dt=i32), o_keep=z(B, dt=i32), flags=z(1, dt=i32))
        self._ctraj = _CTraj(*[self.traj[n].data_ptr() for n in _FIELDS], self.hist_bound, self.pcap)
        self._alloc_turn_loop()              # (`epoch`: of the guesser's sampler)
        self.o_next_tok, self.o_next_cnt = z(B, dt=i32), z(B, dt=i32)
        self.seeds_d, self.det_d, self.draws_d = z(B, dt=t.int64), z(B, dt=u8), z(B, dt=i32)
        self.mt = z(self._L.lmrl_mt_bytes(B), dt=u8)
        self.bound_d = t.tensor([len(self.word_list)], dtype=i32, device=self.dev)
        self.turn_graphs = {}
        self._answers = None                 # int8 [B][T'] injected answer codes
        self._final = True                   # the host's re-judgement of the flagged turns has been applied to the record

    def close(self):
        if getattr(self, "_tq", None):
            self._L.lmrl_tq_destroy(self._tq)
            self._tq = None

    # ---- scripted workloads ------------------------------------------------------------------------------------------------------------
    def set_scripted_questions(self, texts, strength: float = 30.0) -> None:
        """Synthetic-workload hook (tools, tests; as `ChessRolloutEngine.set_scripted_actions`): `texts` [T][B] of str (None: no steering) — in turn
        t the guesser's sampler of env b is steered (+`strength` on one logit per generated position; every logit is still computed and sampled)
        towards spelling that text and a newline, cut to max_new_tokens ids.  None switches it off.  Captured turn graphs are dropped."""
        self.turn_graphs = {}
        if texts is not None:
            assert len(texts) == self.T and all(len(r) == self.B for r in texts)
            texts = [[None if s is None else self.tok.encode(s + "\n") for s in row] for row in texts]
        self._set_script(texts, strength)

    def set_scripted_answers(self, codes) -> None:
        """The oracle's answer of env b in turn t becomes codes[b][t] (1 "Yes.", 0 "No.", < 0: ask the model; turns past the table repeat its last
        column) whatever the oracle model generates — it still runs.  None: back to the model.  Captured turn graphs are dropped."""
        import torch
        self.turn_graphs = {}
        if codes is None:
            self._answers = None
            return
        codes = np.ascontiguousarray(codes, dtype=np.int8)
        assert codes.ndim == 2 and codes.shape[0] == self.B and codes.shape[1] >= 1
        self._answers = torch.from_numpy(codes).to(self.dev)

    # ---- weights -----------------------------------------------------------------------------------------------------------------------
    def set_params(self, engine) -> None:
        """Swap in freshly trained guesser weights (PPOPolicy.set_params, ppo/base_interface.py:821-823)."""
        if type(engine) is not type(self.oeng) or getattr(engine, "matmul", None) != getattr(self.oeng, "matmul", None):
            raise ValueError("TwentyQuestionsRolloutEngine: the guesser's and the oracle's engine must be of one class and one matmul mode")
        self.eng = engine
        self.ses = engine.session(self.B, self.ses.tmax, flags=self.ses.flags)
        self.turn_graphs = {}

    _POLICY = "guesser"

    # ---- one lock-step turn ------------------------------------------------------------------------------------------------------------
    def _feed_guesser(self, n_chunks: int):
        L, sp, tr, B = self._L, _lib.stream_ptr(), ctypes.byref(self._ctraj), self.B
        for j in range(n_chunks):
            _lib.check(L.lmrl_tq_history_chunk(self._tq, tr, j, 16, n_chunks, _lib.ptr(self.chunk_tok), _lib.ptr(self.chunk_cnt), B, sp), "lmrl_tq_history_chunk")
            self.ses.forward(self.chunk_tok, self.chunk_cnt, 16, len_bound_after=self.hist_bound)

    def _turn(self, temperature: float, top_k: int, top_p: float, sample_seed: int, logits_out, first: bool):
        """The whole turn, no host round trip (graph-capturable).  `first`: the oracle's prompt is prefilled from position 0 (more chunks)."""
        L, sp, tr, B = self._L, _lib.stream_ptr(), ctypes.byref(self._ctraj), self.B
        ck = _lib.check
        # host-side bounds only: the device lengths are set by lmrl_tq_question and cannot outgrow the sessions (sized in __init__ for
        # hist_bound + max_new and pcap + oracle_max_new positions; conversations or prompts that would not fit are refused there)
        for ses in (self.ses, self.oses):
            ses._len_bound = 0
        script, g = self._steer_rows(), self.traj
        self._generate(self.ses, (self.ses,), temperature, top_k, top_p, sample_seed, 0.0, _lib.ptr(self.epoch), g["gen_active"], g["out_tok"], g["out_len"],
                       self.next_tok, self.next_cnt, -1 if self.eos is None else int(self.eos), self.max_new, script, logits_out)
        ck(L.lmrl_tq_question(self._tq, tr, 1 if self.reuse_generated else 0, _lib.ptr(self.ses.len), _lib.ptr(self.oses.len), B, sp), "lmrl_tq_question")
        n_chunks = self._o_chunks[0 if first else 1]
        for j in range(n_chunks):
            ck(L.lmrl_tq_oracle_prompt(self._tq, tr, j, 16, n_chunks, _lib.ptr(self.chunk_tok), _lib.ptr(self.chunk_cnt), B, sp), "lmrl_tq_oracle_prompt")
            self.oses.forward(self.chunk_tok, self.chunk_cnt, 16, len_bound_after=self.pcap)
        # the oracle: greedy, eos = the newline (GPT2EngineOracle: do_sample=False)
        self._generate(self.oses, (self.oses,), 0.0, 0, 0.0, 0, 0.0, None, g["o_active"], g["o_out_tok"], g["o_out_len"], self.o_next_tok, self.o_next_cnt,
                       self._oeos, self.omax_new)
        ans = self._answers
        ck(L.lmrl_tq_answer(self._tq, tr, _lib.ptr(ans), int(ans.shape[1]) if ans is not None else 0, B, sp), "lmrl_tq_answer")
        ck(L.lmrl_tq_judge(self._tq, tr, 1 if self.judge == "device" else 0, self.T, B, sp), "lmrl_tq_judge")
        self._feed_guesser(self._g_chunks)
        self._end_turn(script)

    def _reset(self, seeds, options, n_live: Optional[int]):
        """Hidden words (`random.Random(seed)._randbelow(n)` through lmrl_mt_*, or seed % n in deterministic mode), cleared records, and INITIAL_STR
        through the guesser."""
        import torch
        L, sp, B = self._L, _lib.stream_ptr(), self.B
        assert len(seeds) == B
        if options is not None and not isinstance(options, (list, tuple)):
            options = [options] * B
        det = np.asarray([bool((o or {}).get("deterministic", False)) for o in options] if options is not None else [False] * B, dtype=np.uint8)
        if any(s is None or int(s) < 0 or int(s) >= 2 ** 64 for s in seeds):
            raise ValueError("TwentyQuestionsRolloutEngine: every env needs a seed in [0, 2^64) (the generic env draws from an OS-seeded generator otherwise)")
        self.seeds_d.copy_(torch.from_numpy(np.asarray([int(s) for s in seeds], dtype=np.uint64).view(np.int64)))
        self.det_d.copy_(torch.from_numpy(det))
        _lib.check(L.lmrl_mt_seed(_lib.ptr(self.mt), _lib.ptr(self.seeds_d), None, B, sp), "lmrl_mt_seed")
        _lib.check(L.lmrl_mt_randbelow(_lib.ptr(self.mt), _lib.ptr(self.bound_d), _lib.ptr(self.draws_d), 1, B, sp), "lmrl_mt_randbelow")
        _lib.check(L.lmrl_tq_reset(self._tq, ctypes.byref(self._ctraj), _lib.ptr(self.seeds_d), _lib.ptr(self.det_d), _lib.ptr(self.draws_d),
                                   B if n_live is None else int(n_live), _lib.ptr(self.ses.len), _lib.ptr(self.oses.len), B, sp), "lmrl_tq_reset")
        for ses in (self.ses, self.oses):
            ses.reset()
        self._feed_guesser(self._init_chunks)
        self._final = False

    def capture_turns(self, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, sample_seed: int = 0):
        """The two kinds of turn (an episode's first, and the later ones) as hipGraphs; `run_episode(..., use_graph=True)` replays them."""
        self._begin_capture(temperature, top_k, top_p, sample_seed)
        self.turn_graphs = {}
        for first in (True, False) if self.T > 1 else (True,):
            self._reset([0] * self.B, None, None)
            if not first:               # a later turn keeps the oracle prompt's prefix of the turn before it: warm up and capture behind a first turn
                self._turn(temperature, top_k, top_p, sample_seed, self._logits, True)
            self.turn_graphs[first] = self._capture(temperature, top_k, top_p, sample_seed, self._logits, first)
        self._check_flags()
        return self.turn_graphs

    def _graphs(self):
        return self.turn_graphs

    def _recapture(self, temperature, top_k, top_p, sample_seed):
        self.capture_turns(temperature, top_k, top_p, sample_seed)

    def run_episode(self, seeds, options=None, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, sample_seed: int = 0, episode: int = 0,
                    use_graph: bool = False, sync_every: int = 8, max_turns: Optional[int] = None, n_live: Optional[int] = None):
        """One full episode for all B games; returns the device record dict (read after a sync; `records()` / `interactions()` / `ppo_records()`
        apply the host's re-judgement of flagged turns first).  `seeds`: one int per env; `options`: one dict or one per env, `{"deterministic":
        True}` as the env's reset.  The host peeks at the live flags every `sync_every` turns to stop early (0: never)."""
        logits = self._episode_logits(use_graph, temperature, top_k, top_p, sample_seed)
        self._reset(seeds, options, n_live)
        self._start_episode_counters(episode)
        if use_graph:
            return self._run_turns(lambda i: self.turn_graphs[i == 0].replay(), sync_every, max_turns)
        return self._run_turns(lambda i: self._turn(temperature, top_k, top_p, sample_seed, logits, i == 0), sync_every, max_turns)

    # ---- host views --------------------------------------------------------------------------------------------------------------------
    def _check_flags(self):
        f = int(self.traj["flags"].cpu().numpy()[0])
        if f:
            raise _lib.LmrlError(f"TwentyQuestionsRolloutEngine: the last episode outgrew its buffers (flags = {f}: bit 0 oracle chunks, 1 history, "
                                 "2 oracle prompt, 3 guesser chunks)")

    def _finalize(self):
        """The host's half of the judgement: every flagged turn (affirmed, not judged on the device) through `is_done` with the active tagger, in turn
        order; the first one that names the word ends its episode there — reward 0, done, later turns dropped — in the device record itself, so that
        every view (records, interactions, PPO records) sees the cut."""
        import torch
        if self._final:
            return
        self._check_flags()
        flag = self.traj["flag"].cpu().numpy()
        nt = self.traj["n_turns"].cpu().numpy()
        rows = [(b, i) for b in range(self.B) for i in range(int(nt[b])) if flag[b, i]]
        if rows:
            q, ql, word = self.traj["q_text"].cpu().numpy(), self.traj["q_len"].cpu().numpy(), self.traj["word"].cpu().numpy()
            cut = {}
            for b, i in rows:
                if b in cut:
                    continue
                text = q[b, i, : ql[b, i]].tobytes().decode("utf-8")
                if TQ.is_done(self.word_list[int(word[b])], text.strip()):
                    cut[b] = i
            if cut:
                bs = torch.tensor(list(cut), dtype=torch.long, device=self.dev)
                ts = torch.tensor(list(cut.values()), dtype=torch.long, device=self.dev)
                self.traj["reward"][bs, ts] = 0.0
                self.traj["done"][bs, ts] = 1
                self.traj["n_turns"][bs] = (ts + 1).to(torch.int32)
                self.traj["live"][bs] = 0
                keep = torch.arange(self.T, device=self.dev)[None, :] <= ts[:, None]
                self.traj["ep_reward"][bs] = (self.traj["reward"][bs] * keep).sum(1)
        self._final = True

    def records(self):
        """Host copies per game: dict(word index, gen id lists, question texts (bytes as the history holds them), oracle id lists, answer codes,
        reward f32 [n], done bool [n], flag bool [n], live)."""
        self._finalize()
        h = {k: v.cpu().numpy() for k, v in self.traj.items() if k in ("gen", "gen_len", "q_text", "q_len", "ogen", "ogen_len", "answer", "reward", "done", "flag",
                                                                        "n_turns", "live", "ep_reward", "word")}
        out = []
        for b in range(self.B):
            n = int(h["n_turns"][b])
            out.append(dict(word=int(h["word"][b]), gen=[h["gen"][b, i, : h["gen_len"][b, i]].tolist() for i in range(n)],
                            question=[h["q_text"][b, i, : h["q_len"][b, i]].tobytes() for i in range(n)],
                            ogen=[h["ogen"][b, i, : h["ogen_len"][b, i]].tolist() for i in range(n)], answer=h["answer"][b, :n].copy(),
                            reward=h["reward"][b, :n].copy(), done=h["done"][b, :n].astype(bool), flag=h["flag"][b, :n].astype(bool), live=bool(h["live"][b]),
                            ep_reward=float(h["ep_reward"][b])))
        return out

    def interactions(self, n: Optional[int] = None):
        """The finished episodes (of the first `n` games) as `List[List[InteractionTransition]]` — what `interact_environment` returns for the same
        rollouts.  The question texts are decoded on the host from the recorded ids (`out_str_process(tokenizer.decode(ids))`)."""
        from .environment import InteractionTransition, Text
        yes, no = Text("Yes.\n", False), Text("No.\n", False)
        out = []
        for rec in self.records()[: self.B if n is None else int(n)]:
            hist = (Text(TQ.INITIAL_STR, False),)
            trans = []
            for i in range(len(rec["gen"])):
                post_action = hist + (Text(maze_out_str_process(decode_generation(self.tok, rec["gen"][i], self.eos)), True),)
                post = post_action + (yes if rec["answer"][i] else no,)
                trans.append(InteractionTransition(hist, post_action, post, float(rec["reward"][i]), bool(rec["done"][i])))
                hist = post
            out.append(trans)
        return out

    @staticmethod
    def _summary(inter):
        return dict(reward=summarize(np.asarray([sum(t.reward for t in ep) for ep in inter], dtype=np.float32)),
                    done=summarize(np.asarray([ep[-1].done for ep in inter], dtype=np.float32)), length=summarize([len(ep) for ep in inter]))

    def text_env_eval(self, n_rollouts: int, seed_generator=None, env_options=None, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0,
                      sample_seed: int = 0, interaction_callback=None, use_graph: bool = True, sync_every: int = 8):
        """`text_env_eval(env, policy, n_rollouts, bsize=B, env_options=...)` with the lock-step loop on the device: ceil(n / B) episode batches, the
        same (interactions, summary) return value.  The sampler's episode word keeps counting across calls."""
        inter = self._eval_round(n_rollouts, seed_generator, env_options, interaction_callback,
                                 dict(temperature=temperature, top_k=top_k, top_p=top_p, sample_seed=sample_seed, use_graph=use_graph, sync_every=sync_every))
        return inter, self._summary(inter)

    # ---- the online-RL hand-over -------------------------------------------------------------------------------------------------------
    def ppo_records(self, n: Optional[int] = None):
        """The finished episodes (of the first `n` games; default all) as `algorithms.ppo_device.PPORecords`: ONE token trajectory per episode, no
        chains — the whole history's ids, the questions' tokens as actions, each turn's reward on its question's last token, the episode's done — as
        the PPO script builds it from `raw_result[-1].post_transition_history` (twenty_questions/ppo/train_ppo.py:322-352), so that
        `ppo_device.truncate_turns` (the script's drop-the-last-turns rule) and `ppo_data_from_records` apply unchanged."""
        import torch
        from .algorithms.ppo_device import PPORecords
        t = torch
        self._finalize()
        B = self.B if n is None else int(n)
        if int(self.traj["n_turns"][:B].min().item()) <= 0:
            raise ValueError("ppo_records: an env without a recorded turn (run an episode first)")
        cap = self.hist_bound
        tokens, ia, rw = t.zeros(B, cap, dtype=t.int32, device=self.dev), t.zeros(B, cap, dtype=t.uint8, device=self.dev), t.zeros(B, cap, dtype=t.float32, device=self.dev)
        n_tok, done = t.zeros(B, dtype=t.int32, device=self.dev), t.zeros(B, dtype=t.uint8, device=self.dev)
        _lib.check(self._L.lmrl_tq_ppo_records(self._tq, ctypes.byref(self._ctraj), B, cap, _lib.ptr(tokens), _lib.ptr(ia), _lib.ptr(rw), _lib.ptr(n_tok),
                                               _lib.ptr(done), _lib.stream_ptr()), "lmrl_tq_ppo_records")
        return PPORecords(tokens, ia, rw, n_tok, done)

    def ppo_data(self, inference, *, gamma: float, lam: float, kl_weight: float, max_length: Optional[int] = None, n: Optional[int] = None,
                 truncate: bool = True, **kw):
        """`ppo_dataset_loader` of the PPO script on the episodes this engine just ran -> (DevicePPODataset, all_kls).  `truncate` (with a
        `max_length`): the script's rule first — while a trajectory has more than three texts and at least max_length tokens its last (question,
        answer) pair is dropped (`ppo_device.truncate_turns`)."""
        from .algorithms.ppo_device import ppo_data_from_records, truncate_turns
        rec = self.ppo_records(n)
        if truncate and max_length is not None:
            rec, self.last_truncation = truncate_turns(rec, int(max_length), float(gamma))
        return ppo_data_from_records(inference, rec, gamma=gamma, lam=lam, kl_weight=kl_weight, max_length=max_length, **kw)

    def ppo_rollouts(self, inference, n_rollouts: int, seed_generator=None, env_options=None, *, gamma: float, lam: float, kl_weight: float,
                     max_length: Optional[int] = None, use_advantage_whitening: bool = True, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0,
                     sample_seed: int = 0, use_graph: bool = True, **kw):
        """One data-collection round of the PPO loop on the device: `text_env_eval(n_rollouts, bsize=B)` + `ppo_dataset_loader` ->
        (DevicePPODataset over all rollouts, all_kls, summary).  Per episode batch: the lock-step episode, then its PPO data while the record is in
        the engine's buffers; advantages whitened once over the action tokens of the whole round; `summary` has `text_env_eval`'s fields."""
        return self._ppo_round(inference, n_rollouts, seed_generator, env_options, use_advantage_whitening,
                               dict(temperature=temperature, top_k=top_k, top_p=top_p, sample_seed=sample_seed, use_graph=use_graph),
                               dict(gamma=gamma, lam=lam, kl_weight=kl_weight, max_length=max_length, **kw))

    def _round_stats(self, actual: int):
        nt = self.traj["n_turns"][:actual].cpu().numpy()
        dn = self.traj["done"][:actual].cpu().numpy()
        return np.stack([self.traj["ep_reward"][:actual].cpu().numpy().astype(np.float64), dn[np.arange(actual), np.maximum(nt - 1, 0)].astype(np.float64),
                         nt.astype(np.float64)])
