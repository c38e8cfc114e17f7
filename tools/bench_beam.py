"""Beam decoding on the device vs the same rows decoded greedily: GPT-2-small, B = 32 prompts of 256 tokens, K = 4 beams, 32 new tokens.

    python tools/bench_beam.py [--reps 5]

Prints one JSON line: tokens/s of beam decoding (B * K rows x positions run), the per-position time of the three new launches
(lmrl_beam_row_topk, lmrl_beam_select, lmrl_gpt2_kv_reorder), and tokens/s of the same B * K rows decoded greedily in an ordinary session with
the prompts duplicated (existing code: a commit without beam search can run that leg with --greedy-only)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--greedy-only", type=int, default=0)
    a = ap.parse_args()
    import torch
    import lmrl_gym_amd  # noqa: F401
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine
    from lmrl_gym_amd.policies import _Generator
    dev = _lib.require_gpu()
    cfg = GPT2Config.gpt2_small()
    eng = GPT2Engine.random_init(cfg, seed=0, device=dev)
    B, K, P, T = 32, 4, 256, 32
    rng = np.random.RandomState(0)
    prompts = [rng.randint(0, cfg.vocab, size=P).tolist() for _ in range(B)]
    tmax = P + T + 16
    out = dict(config=dict(model="gpt2-small", B=B, K=K, prompt_tokens=P, new_tokens=T))

    # ---- greedy: B * K rows, prompts duplicated, ordinary session
    from lmrl_gym_amd.gpt2 import SampleParams
    gen = _Generator([eng], B * K, tmax)
    dup = [p for p in prompts for _ in range(K)]
    L = _lib.lib()
    R = B * K

    def greedy():
        gen.prefill(dup, reuse=False)
        ses = gen.sessions[0]
        active = torch.ones(R, dtype=torch.uint8, device=dev)
        out_tok = torch.zeros(R, T, dtype=torch.int32, device=dev)
        out_len, nt, nc = (torch.zeros(R, dtype=torch.int32, device=dev) for _ in range(3))
        for k in range(T):
            tok, _ = ses.sample(SampleParams(0.0, 0, 0, k, 0.0, 0.0, 0, None, 0.0, 0, 0), active=active, want_logprob=False)
            _lib.check(L.lmrl_gen_accept(_lib.ptr(tok), _lib.ptr(active), _lib.ptr(out_tok), _lib.ptr(out_len), _lib.ptr(nt), _lib.ptr(nc), -1, T, R,
                                         _lib.stream_ptr()), "lmrl_gen_accept")
            if k + 1 < T:
                ses.forward(nt, nc, 1)
        torch.cuda.synchronize()

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return float(np.median(ts))
    tg = timed(greedy)
    out["greedy_duplicated_prompts"] = dict(seconds=tg, tokens_per_s=R * T / tg)
    if not a.greedy_only:
        from lmrl_gym_amd.beam import BeamSearch, kv_reorder
        bs = BeamSearch([eng], B, K, tmax, eos_token_id=None)
        tb = timed(lambda: (bs.run(prompts, T, reuse=False), torch.cuda.synchronize()))
        out["beam"] = dict(seconds=tb, positions=bs.steps, tokens_per_s=R * bs.steps / tb)
        # the three new launches at the state the search left (position T - 1 sizes: the longest suffix)
        st, ctl = bs._states, bs._ctl
        ctl[0].fill_(1)
        pair = bs.beams[0]
        lg = bs.logits
        ev = lambda: torch.cuda.Event(enable_timing=True)

        def per_launch(fn, n=50):
            fn(); torch.cuda.synchronize()
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(n):
                fn()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n
        sp = _lib.stream_ptr()
        t_row = per_launch(lambda: _lib.check(L.lmrl_beam_row_topk(_lib.ptr(lg), lg.shape[1], R, cfg.vocab, 2 * K, _lib.ptr(st[0].run_score), None, ctl.data_ptr(),
                                                                   _lib.ptr(bs.cand_score), _lib.ptr(bs.cand_tok), sp), "lmrl_beam_row_topk"))
        tick = ctl[1:].clone()

        def sel():
            ctl[1:].copy_(tick)
            _lib.check(L.lmrl_beam_select(ctypes.byref(st[0].c), ctypes.byref(st[1].c), _lib.ptr(bs.cand_score), _lib.ptr(bs.cand_tok), _lib.ptr(bs.parent),
                                          _lib.ptr(bs.next_tok), _lib.ptr(bs.next_cnt), _lib.ptr(ctl), B, K, cfg.vocab, bs._cap, T - 2, T, -1, 0, 0, K - 1, 1.0, 1.0, sp),
                       "lmrl_beam_select")
        ctl[1:].zero_(); tick.zero_()
        t_sel = per_launch(sel) - per_launch(lambda: ctl[1:].copy_(tick))
        t_reo = per_launch(lambda: kv_reorder(pair[0], pair[1], bs.parent, ctl.data_ptr()))
        out["new_launches_us"] = dict(row_topk=t_row, select=t_sel, kv_reorder_at_last_position=t_reo)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
