"""Beam search on the device for the GPT-2 policies — `num_beams` of the reference's `GenerationConfig`
(llm_rl_scripts/wordle/ppo/train_ppo_gpt2.py:96,219, every eval_* script's `--policy-num-beams`).

The rules are those of HF-Flax `_beam_search` as transformers 4.26.1 (the reference's pin) runs it, RESTATED in DESIGN.md ("Beam search") and
unverified against the library itself, which is not installed; where the installed torch transformers differs (it normalises by generated
length and stops by another heuristic) the restatement holds.  `tests/beam_oracle.py` is the same restatement in numpy float64.

Design: the B prompts are prefilled ONCE into an ordinary B-row session per engine (`_Generator.prefill`, with prefix reuse across calls); two
B * K-row sessions per engine are attached to it (`attach_prefix_from`, row b * K + k -> prompt b), so the K beams of an item read one copy of
the prompt's K/V rows in place.  Per generated position: logits of the B * K rows (the existing LM-head / value-head entries) ->
`lmrl_beam_row_topk` -> `lmrl_beam_select` -> `lmrl_*_kv_reorder` of the generated suffix into the other attached session by `parent` -> a
single-token forward there.  Nothing of a step runs on the host; the host peeks at the device's `go` word every 16 positions.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .gpt2 import FWD_RAGGED_ALWAYS, RNG_PHILOX, SAMPLE_WANT_LOGITS, SampleParams

NEG = -1.0e7
# `best_running = running_score[BEST_RUNNING_BEAM] / max_length ** length_penalty` of the loop condition: that release reads the LAST running beam
# (`running_scores[:, -1:]`), not the first.  One constant for the kernel side and the oracle (tests/beam_oracle.py imports it).
BEST_RUNNING_BEAM = -1
MAX_BEAMS = 16          # lmrl_beam_select: 2 K <= 32 candidates per row


class _CBeamState(ctypes.Structure):     # lmrl_beam_state (include/lmrl_amd.h)
    _fields_ = [("run_score", ctypes.c_void_p), ("run_hist", ctypes.c_void_p), ("fin_score", ctypes.c_void_p), ("fin_flag", ctypes.c_void_p),
                ("fin_hist", ctypes.c_void_p)]


class _State:
    def __init__(self, t, rows, cap, dev):
        self.run_score = t.zeros(rows, dtype=t.float32, device=dev)
        self.run_hist = t.zeros(rows, cap, dtype=t.int32, device=dev)
        self.fin_score = t.zeros(rows, dtype=t.float32, device=dev)
        self.fin_flag = t.zeros(rows, dtype=t.uint8, device=dev)
        self.fin_hist = t.zeros(rows, cap, dtype=t.int32, device=dev)
        self.c = _CBeamState(*(_lib.ptr(x) for x in (self.run_score, self.run_hist, self.fin_score, self.fin_flag, self.fin_hist)))


def kv_reorder(src, dst, parent, go_ptr: Optional[int] = None) -> None:
    """Row i of the attached session `dst` continues row parent[i] (int32 device tensor, absolute rows) of the attached session `src` of the same
    engine, shape and prefix: K/V of the generated positions, cache length, last hidden state (fp32 engine: and last residual).  `go_ptr`: device
    address of an int32 word; 0 there: nothing is written."""
    e = src.eng
    assert dst.eng is e and dst.B == src.B and dst.tmax == src.tmax and src is not dst
    if src._prefix is None or dst._prefix is None:
        raise _lib.LmrlError("kv_reorder: both sessions must be attached to a prompt-prefix session (attach_prefix_from)")
    if hasattr(e, "_h"):
        _lib.check(e._L.lmrl_gpt2_kv_reorder(e._h, _lib.ptr(src.kv), _lib.ptr(src.len), _lib.ptr(src.last_hidden), _lib.ptr(parent), _lib.ptr(src._pfx_n),
                                             _lib.ptr(dst.kv), _lib.ptr(dst.len), _lib.ptr(dst.last_hidden), src.B, src.tmax, go_ptr, _lib.stream_ptr()),
                   "lmrl_gpt2_kv_reorder")
    else:
        c = e.cfg
        _lib.check(e._L.lmrl_kv_reorder_f32(_lib.ptr(src.kv), _lib.ptr(src.len), _lib.ptr(src.last_hidden), _lib.ptr(src._last_x), _lib.ptr(parent),
                                            _lib.ptr(src._pfx_n), _lib.ptr(dst.kv), _lib.ptr(dst.len), _lib.ptr(dst.last_hidden), _lib.ptr(dst._last_x),
                                            src.B, src.tmax, c.n_layer, c.d_model, go_ptr, _lib.stream_ptr()), "lmrl_kv_reorder_f32")
    dst._len_bound = src._len_bound


class BeamSearch:
    """Beam search of width `num_beams` for a fixed batch on one engine (PPO / BC policy) or on two engines plus Q heads (the value policy:
    logits = pi_beta + beta * min(Q1, Q2), `q_heads = (q1, q2 or None)` in the engines' head layout).  `GPT2Engine` and `GPT2EngineF32` (both
    matmul modes)."""

    def __init__(self, engines: Sequence, batch: int, num_beams: int, tmax: int, q_heads=None, beta: float = 0.0, length_penalty: float = 1.0,
                 early_stopping: bool = False, eos_token_id: Optional[int] = None, pad_token_id: int = 0):
        import torch
        from .policies import _Generator
        if not 1 <= num_beams <= MAX_BEAMS:
            raise _lib.LmrlError(f"num_beams = {num_beams}: 1 .. {MAX_BEAMS}")
        self.t = torch
        self.engines, self.B, self.K, self.tmax = list(engines), batch, num_beams, tmax
        if (q_heads is not None) != (len(self.engines) == 2):
            raise _lib.LmrlError("BeamSearch: one engine, or two engines (pi_beta, value base) with q_heads")
        self.q_heads, self.beta = q_heads, float(beta)
        self.length_penalty, self.early_stopping = float(length_penalty), bool(early_stopping)
        self.eos, self.pad = eos_token_id, int(pad_token_id)
        self.cfg = self.engines[0].cfg
        if self.cfg.vocab < 2 * num_beams:
            raise _lib.LmrlError(f"num_beams = {num_beams} needs a vocabulary of at least {2 * num_beams} tokens")
        self.gen = _Generator(self.engines, batch, tmax)          # the prompts: one row each, prefix reuse across calls
        self.dev = self.gen.dev
        R = batch * num_beams
        self.rows = R
        self.beams = [[e.session(R, tmax, flags=FWD_RAGGED_ALWAYS) for _ in range(2)] for e in self.engines]
        self.idx = torch.arange(R, dtype=torch.int32, device=self.dev) // num_beams          # row b * K + k stands on prompt b
        self.logits = torch.zeros(R, self.cfg.vocab_padded, dtype=torch.float32, device=self.dev)
        self.cand_score = torch.zeros(R, 2 * num_beams, dtype=torch.float32, device=self.dev)
        self.cand_tok = torch.zeros(R, 2 * num_beams, dtype=torch.int32, device=self.dev)
        self.parent = torch.zeros(R, dtype=torch.int32, device=self.dev)
        self.next_tok = torch.zeros(R, dtype=torch.int32, device=self.dev)
        self.next_cnt = torch.zeros(R, dtype=torch.int32, device=self.dev)
        self._cap, self._states, self._ctl = 0, None, None
        if q_heads is not None:
            vb = self.engines[1]
            self.qh, self.q_ws = [vb.q_hidden_buffer(R) for _ in range(2)], vb.q_hidden_ws(R)

    @property
    def prefilled_tokens(self) -> int:
        return self.gen.prefilled_tokens

    def _logits(self, cur):
        """Logits [B K][vocab_padded] of the current sessions' last tokens, through the existing entries (no warper applies under beam search)."""
        pi = cur[0]
        f32 = getattr(pi.eng, "matmul", None) == "f32"
        if f32 and self.q_heads is None:
            return pi.lm_logits()
        p = SampleParams(0.0, 0, 0, 0, 0.0, self.beta, self.pad, None, 0.0, RNG_PHILOX, SAMPLE_WANT_LOGITS)
        ops = [None, None]
        if self.q_heads is not None:
            vb, v_ses = self.engines[1], cur[1]
            for i, head in enumerate(self.q_heads):
                if head is None:
                    continue
                vb.q_hidden(head, v_ses.last_hidden, self.qh[i], self.q_ws)
                ops[i] = (self.qh[i], head.get("w2_x3", head["w2"]), head["b2"])
        if f32:
            pi.sample(p, q1=ops[0], q2=ops[1], want_logprob=False)         # materialises pi.logits (lmrl_value_head_logits_f32)
            return pi.logits
        pi.sample(p, logits_out=self.logits, q1=ops[0], q2=ops[1], want_logprob=False)
        return self.logits

    def run(self, prompts: List[List[int]], max_new_tokens: int, prompt_width: Optional[int] = None, reuse: bool = True, trace: Optional[list] = None):
        """prompts: B token lists.  prompt_width: the padded prompt width P of the rules (the scripts' blocking strategy pads every row to
        `max_input_length`); default: the longest prompt.  Returns (sequences, scores): per item the generated ids of the best hypothesis, cut
        behind the first eos, and its score.  trace (tests only): a list that receives, per position, the host copies of the logits and of the
        step's outputs — one device sync per position."""
        t, L, B, K, R, T = self.t, _lib.lib(), self.B, self.K, self.rows, int(max_new_tokens)
        assert len(prompts) == B and T >= 1
        P = int(prompt_width) if prompt_width is not None else max(len(p) for p in prompts)
        if max(len(p) for p in prompts) + T > self.tmax:
            raise _lib.LmrlError(f"KV cache overflow: prompt + {T} new tokens into a cache of tmax = {self.tmax}")
        self.gen.prefill(prompts, reuse=reuse)
        max_pos = max(len(p) for p in prompts)
        for src, pair in zip(self.gen.sessions, self.beams):
            for s in pair:
                s.attach_prefix_from(src, self.idx, max_pos, group=True)
        if self._cap < T:
            self._cap = T
            self._states = [_State(t, R, T, self.dev) for _ in range(2)]
            self._ctl = t.zeros(4, T + 1, dtype=t.int32, device=self.dev)
        cap, st, ctl = self._cap, self._states, self._ctl
        for s in st:
            s.run_hist.fill_(self.pad); s.fin_hist.fill_(self.pad); s.fin_score.zero_(); s.fin_flag.zero_()
        st[0].run_score.copy_(t.tensor([0.0] + [NEG] * (K - 1), dtype=t.float32).repeat(B))
        ctl.zero_()
        ctl[0, 0] = 1
        go_ptr = lambda i: ctl.data_ptr() + 4 * i
        eos = -1 if self.eos is None else int(self.eos)
        best = BEST_RUNNING_BEAM % K
        best_div = float(P + T) ** self.length_penalty
        sp = _lib.stream_ptr()
        cur = 0
        for i in range(T):
            if i % 16 == 0 and i > 0 and int(ctl[0, i].item()) == 0:
                break
            ses = [pair[cur] for pair in self.beams]
            lg = self._logits(ses)
            _lib.check(L.lmrl_beam_row_topk(_lib.ptr(lg), lg.shape[1], R, self.cfg.vocab, 2 * K, _lib.ptr(st[cur].run_score), None, go_ptr(i),
                                            _lib.ptr(self.cand_score), _lib.ptr(self.cand_tok), sp), "lmrl_beam_row_topk")
            _lib.check(L.lmrl_beam_select(ctypes.byref(st[cur].c), ctypes.byref(st[1 - cur].c), _lib.ptr(self.cand_score), _lib.ptr(self.cand_tok),
                                          _lib.ptr(self.parent), _lib.ptr(self.next_tok), _lib.ptr(self.next_cnt), _lib.ptr(ctl), B, K, self.cfg.vocab, cap,
                                          i, T, eos, self.pad, int(self.early_stopping), best, float(P + i) ** self.length_penalty, best_div, sp),
                       "lmrl_beam_select")
            if trace is not None:
                o = st[1 - cur]
                trace.append(dict(go=int(ctl[0, i].item()), logits=lg[:, : self.cfg.vocab].cpu().numpy().copy(), parent=self.parent.cpu().numpy().copy(),
                                  tok=self.next_tok.cpu().numpy().copy(), run_score=o.run_score.cpu().numpy().copy(),
                                  fin_score=o.fin_score.cpu().numpy().copy(), fin_flag=o.fin_flag.cpu().numpy().copy(),
                                  fin_hist=o.fin_hist.cpu().numpy().copy(), run_hist=o.run_hist.cpu().numpy().copy()))
            if i + 1 < T:
                for pair in self.beams:
                    kv_reorder(pair[cur], pair[1 - cur], self.parent, go_ptr(i + 1))
                    pair[1 - cur].forward(self.next_tok, self.next_cnt, 1)
            cur = 1 - cur
        go = ctl[0, :T].cpu().numpy()
        n = int((go != 0).sum())                       # positions that ran (a prefix of ones)
        assert n >= 1 and bool((go[:n] != 0).all())
        self.steps = n
        fs = st[n % 2]
        run_hist, run_score = fs.run_hist.cpu().numpy().reshape(B, K, cap), fs.run_score.cpu().numpy().reshape(B, K)
        fin_hist, fin_score, fin_flag = fs.fin_hist.cpu().numpy().reshape(B, K, cap), fs.fin_score.cpu().numpy().reshape(B, K), fs.fin_flag.cpu().numpy().reshape(B, K)
        seqs, scores = [], np.zeros(B, dtype=np.float32)
        for b in range(B):
            if fin_flag[b].any():                      # flagged entries stand before unflagged ones: entry 0 is the best finished hypothesis
                ids, scores[b] = fin_hist[b, 0, :n].tolist(), fin_score[b, 0]
            else:
                ids, scores[b] = run_hist[b, 0, :n].tolist(), run_score[b, 0]
            if eos >= 0 and eos in ids:
                ids = ids[: ids.index(eos) + 1]
            seqs.append(ids)
        return seqs, scores
