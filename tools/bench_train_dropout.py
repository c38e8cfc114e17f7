"""Cost of dropout in the ILQL train step: GPT-2-small, B = 32 x T = 512 (the workload of `bench.py --mode ilql-step`), in
both arithmetic modes, rates 0 against 0.1 on all three sites (the reference's ILQL default, via HF GPT2Config) and, to separate the sites, 0.1
on one kind of site at a time.  Every case is timed `--repeats` times in interleaved order (case A, B, C, ..., then again) after a warm-up, with
a device synchronisation around each timed group of `--steps` steps; the line reports the median and the spread (max - min) of the repeats, so
a difference smaller than the spread is not a finding.  Prints ONE JSON line.
usage: python tools/bench_train_dropout.py [--steps K] [--repeats R] [--bsize B] [--modes f32,bf16] [--sites 0|1]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lmrl_gym_amd  # noqa: F401
from lmrl_gym_amd import _lib, jax_prng
from lmrl_gym_amd.algorithms import ilql
from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, MLPHeadF32


def make_step(dev, cfg, sd, mode, rates, B, T):
    d, V, pad = cfg.d_model, cfg.vocab, 50257
    base, tbase = GPT2F32(sd, cfg.n_head, device=dev, matmul=mode, **rates), GPT2F32(sd, cfg.n_head, device=dev, matmul=mode, **rates)
    g = torch.Generator().manual_seed(1)
    mk = lambda out: MLPHeadF32({"dense1.kernel": torch.randn(d, d, generator=g) * 0.02, "dense1.bias": torch.zeros(d),
                                 "dense2.kernel": torch.zeros(d, out), "dense2.bias": torch.full((out,), -4.4)}, dev, matmul=mode)
    tr = ilql.GPT2ILQLTrain(base, mk(V), mk(V), mk(1), pad, dict(gamma=0.99, tau=0.7, cql_weight=0.01), target_base=tbase, lr=3e-5)
    rng = np.random.RandomState(1000)
    ids = rng.randint(0, 50257, size=(B, T)).astype(np.int32)
    t = np.arange(T - 1)
    sta = np.broadcast_to(((t >= 4) & (((t - 4) // 6) % 2 == 0))[None, :], (B, T - 1)).copy()
    rewards = np.where(sta & ~np.roll(sta, -1, axis=1), -1.0, 0.0).astype(np.float32)
    dones = (rng.rand(B) < 0.5).astype(np.float32)
    keys = jax_prng.StepKeys(jax_prng.prng_key(0) if rates else None)
    return lambda: tr.step(ids, sta, rewards, dones, prng_key=keys.next())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bsize", type=int, default=32)
    ap.add_argument("--modes", default="f32,bf16")
    ap.add_argument("--sites", type=int, default=1, help="1: also time each kind of site alone")
    a = ap.parse_args()
    dev = _lib.require_gpu()
    cfg = GPT2Config.gpt2_small(50258)
    sd = init_hf_style_state_dict(cfg, seed=0)
    cases = {"p0": {}, "p0.1": dict(embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1)}
    if a.sites:
        cases.update({"embd0.1": dict(embd_pdrop=0.1), "attn0.1": dict(attn_pdrop=0.1), "resid0.1": dict(resid_pdrop=0.1)})
    out = dict(workload="ILQL step, GPT-2-small, B=%d x T=512" % a.bsize, steps=a.steps, repeats=a.repeats, device=torch.cuda.get_device_name(dev), ms={})
    for mode in a.modes.split(","):
        times = {k: [] for k in cases}
        for name, rates in cases.items():          # one case resident at a time: five ILQL trainers do not fit side by side with their workspaces
            step = make_step(dev, cfg, sd, mode, rates, a.bsize, 512)
            step(); step()
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            del step
            torch.cuda.empty_cache()
        out["ms"][mode] = {k: dict(median=round(float(np.median(v)), 2), spread=round(max(v) - min(v), 2)) for k, v in times.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
