"""Throughput of the device-resident chess rollout loop against the generic text path on the same workload and the same box.

    python tools/bench_chess_device.py [--envs 1024] [--host-envs 1024,256] [--max-moves 5] [--max-new 8] [--runs 3]

GPT-2-small (random weights), the byte tokenizer, `large_piece_random_endgame("kQK")` start positions, a random opponent.  Three legs, one JSON line:

  device_scripted   `ChessRolloutEngine` under graph replay, the sampler steered towards legal-ish SAN strings (queen / king moves of the start
                    position and a few common squares), device opponent: games with real moves, replies and early ends
  device            the same engine, unsteered: the policy samples from its random weights at temperature 1 — exactly the workload of the next leg
  host              `E.text_env_eval(VectorChessEnv(random_opponent=True), GPT2PPOPolicy)`: today's path (FEN text down, tokenizer, pad, prefill,
                    decode, action strings up)

An env-step is one agent turn of one live game; every leg reports env-steps/s over `--runs` timed runs after a warm-up (median, and each run).
`ratio` = device / host at the same number of envs; `host_noreuse` / `ratio_noreuse`: the host policy with `reuse_kv=False` (it then prefills
every turn from position 0 as the device loop does; by default it keeps the K/V rows of the longest common prefix of consecutive prompts).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--host-envs", default="1024,256", help="batch sizes of the host leg (each is also run on the device)")
    ap.add_argument("--max-moves", type=int, default=5)
    ap.add_argument("--max-new", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--model", default="small", choices=["tiny", "small"])
    a = ap.parse_args(argv)
    import torch
    import lmrl_gym_amd  # noqa: F401
    from lmrl_gym_amd import _lib, environment as E
    from lmrl_gym_amd.chess_rollout import ChessRolloutEngine
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.envs import chess as C
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine, init_hf_style_state_dict
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    dev = _lib.require_gpu()
    tok = ByteTokenizer()
    cfg = GPT2Config.gpt2_small(50257) if a.model == "small" else GPT2Config(2, 2, 128, 256, 50257, 256)
    engine = GPT2Engine(cfg, init_hf_style_state_dict(cfg, seed=0), dev)
    sizes = sorted({a.envs} | {int(x) for x in a.host_envs.split(",") if x}, reverse=True)
    np.random.seed(0)
    all_starts = [C.large_piece_random_endgame("kQK") for _ in range(max(sizes))]
    prompt_bound = -(-max(2 * len(s) + 9 for s in all_starts) // 16) * 16       # kQK positions: the counters may grow by a few digits
    out = dict(model=a.model, max_moves=a.max_moves, max_new_tokens=a.max_new, runs=a.runs, prompt_bound=prompt_bound, legs=[])

    def timed(fn):
        fn()                                        # warm-up (graph capture, allocations)
        torch.cuda.synchronize()
        rates = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            steps = fn()
            torch.cuda.synchronize()
            rates.append(steps / (time.perf_counter() - t0))
        return rates

    for B in sizes:
        starts = all_starts[:B]
        options = [dict(from_position=s) for s in starts]
        env = C.VectorChessEnv(max_moves=a.max_moves, random_opponent=True)
        eng = ChessRolloutEngine(engine, tok, env, B, max_new_tokens=a.max_new, eos_token_id=tok.encode("\n")[0], max_input_length=256,
                                 prompt_bound=prompt_bound)
        rng = random.Random(1)
        L = _lib.lib()
        import ctypes

        def legal(fen):
            buf = ctypes.create_string_buffer(L.lmrl_chess_pos_bytes())
            L.lmrl_chess_host_from_fen(fen.encode(), buf)
            u, s = ctypes.create_string_buffer(256 * 8), ctypes.create_string_buffer(256 * 16)
            k = L.lmrl_chess_host_legal_moves(buf, u, s)
            return [s.raw[i * 16:(i + 1) * 16].split(b"\0")[0].decode() for i in range(k)]
        pools = [[m for m in legal(s) if len(m) <= (a.max_new - 1) // 2 + 1] or ["Kd4"] for s in starts]
        script = [[rng.choice(pools[b]) for b in range(B)] for _ in range(eng.T)]
        episode = [0]

        def device_run():
            eng.run_episode([0] * B, options, temperature=1.0, sample_seed=3, episode=episode[0], use_graph=True, sync_every=0)
            episode[0] += 1
            return int(eng.traj["n_turns"].sum().item())
        for name, sc in (("device_scripted", script), ("device", None)):
            eng.set_scripted_actions(sc, strength=30.0)
            rates = timed(device_run)
            res = np.bincount(np.concatenate([r["result"] for r in eng.records()]), minlength=4).tolist()
            out["legs"].append(dict(leg=name, envs=B, env_steps_per_s=float(np.median(rates)), runs=[float(x) for x in rates], results_last_run=res))
        eng.close()
        if str(B) in a.host_envs.split(","):
            # host: the policy as the harness builds it (reuse_kv=True: the K/V rows of the longest common prefix of consecutive prompts are kept —
            # on a game whose position does not change, i.e. after an illegal move, that is the whole prompt); host_noreuse: every turn prefills
            # from position 0, the device loop's schedule
            for name, reuse in (("host", True), ("host_noreuse", False)):
                pol = GPT2PPOPolicy(engine, tok, max_input_length=256, max_new_tokens=a.max_new, do_sample=True, temperature=1.0,
                                    eos_token_id=tok.encode("\n")[0], out_str_process=lambda x: x.removesuffix("\n") + "\n", reuse_kv=reuse)

                def host_run():
                    inter = E.interact_environment(env, pol, env_seed=[None] * B, env_options=options, bsize=B)
                    return sum(len(ep) for ep in inter)
                rates = timed(host_run)
                out["legs"].append(dict(leg=name, envs=B, env_steps_per_s=float(np.median(rates)), runs=[float(x) for x in rates]))
        env.close()
    by = {(l["leg"], l["envs"]): l["env_steps_per_s"] for l in out["legs"]}
    out["ratio"] = {str(B): by[("device", B)] / by[("host", B)] for B in sizes if ("host", B) in by}
    out["ratio_noreuse"] = {str(B): by[("device", B)] / by[("host_noreuse", B)] for B in sizes if ("host_noreuse", B) in by}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
