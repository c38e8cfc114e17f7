"""Records -> blocked ILQL dataset: episodes/s of
  (host)   `ScriptedRecords.to_items()` -> tokenizer -> `ILQLData.from_token_trajectory_chain` -> `ILQLDataset.from_ilql_data_list`
           (what `ilql_dataset_from_jsonl` does with a generated file; the readback of the records is included, file I/O is not),
  (device) `WordleScriptedRollouts.token_records()` -> `offline_device.ilql_data_from_records`, with HIP-event times per phase,
on the same episodes of the 431-word list, plus the MC and BC builds of the device path.  One JSON line.

    python tools/bench_offline_data.py [--episodes 16384] [--vocab wordle_official_400.txt] [--prob-smart 0.5] [--max-length 512] [--reps 7]

With --step 1 (default) it also times `GPT2ILQLTrain.step` at GPT-2-small shapes, B = 32 x T = 512, bf16-matmul mode, once from a numpy batch
(the host dataset's rows) and once from a device batch (`DeviceILQLDataset.batch`): wall-clock milliseconds per step including the batch's
way to the step, median of --reps after two warm steps.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ilql_step_ms(ds, reps):
    import numpy as np
    import torch
    from lmrl_gym_amd.algorithms import ilql
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, MLPHeadF32
    dev = ds.input_ids.device
    cfg = GPT2Config(12, 12, 768, 3072, 50258, 1024)
    sd = init_hf_style_state_dict(cfg, seed=0)
    g = torch.Generator().manual_seed(1)
    d, V = cfg.d_model, cfg.vocab
    mk = lambda out: MLPHeadF32({"dense1.kernel": torch.randn(d, d, generator=g) * 0.02, "dense1.bias": torch.zeros(d),
                                 "dense2.kernel": torch.randn(d, out, generator=g) * 0.02, "dense2.bias": torch.zeros(out)}, dev, matmul="bf16")
    base = GPT2F32(sd, cfg.n_head, device=dev, matmul="bf16")
    tr = ilql.GPT2ILQLTrain(base, mk(V), mk(V), mk(1), 50257, dict(gamma=0.99, tau=0.7, cql_weight=0.01), lr=1e-5)
    host = ds.to_host()
    rng = np.random.default_rng(3)
    res = {}
    for kind in ("numpy_batch", "device_batch"):
        ms = []
        for it in range(reps + 2):
            index = rng.permutation(len(ds))[:32]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch = host[index] if kind == "numpy_batch" else ds.batch(index)
            tr.step(**batch)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[kind + "_ms"] = sorted(ms[2:])[len(ms[2:]) // 2]
    res.update(B=32, T=int(ds.input_ids.shape[1]), model="gpt2-small shapes, bf16-matmul mode")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=16384)
    ap.add_argument("--vocab", default="wordle_official_400.txt")
    ap.add_argument("--prob-smart", type=float, default=0.5)
    ap.add_argument("--max-length", type=int, default=512)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", type=int, default=1, help="1: also time the GPT-2-small ILQL step at B = 32 x T = 512 from a numpy and from a device batch")
    a = ap.parse_args()
    import numpy as np
    import torch
    from lmrl_gym_amd import datasets as DS
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.algorithms import offline_device as OD
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ilql import ILQLData, ILQLDataset
    from lmrl_gym_amd.envs import wordle as W, wordle_policies as P
    vocab = W.Vocabulary.builtin(a.vocab)
    n = a.episodes
    loop = P.WordleScriptedRollouts(vocab, P.RandomMixturePolicy(a.prob_smart, vocab), n)
    rng = np.random.default_rng(0)
    loop.run_device(rng.integers(0, 2 ** 31 - 1, n).tolist(), rng.integers(0, 2 ** 31 - 1, n).tolist())
    torch.cuda.synchronize()
    tok = DS.WordleTokenizer()
    bs = BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, a.max_length)
    out = dict(bench="offline_data", vocab=a.vocab, n_words=vocab.all_vocab_size(), episodes=n, max_length=a.max_length, reps=a.reps)

    # ---- host path
    t0 = time.perf_counter()
    items = loop.records().to_items()
    t1 = time.perf_counter()
    chains = [E.TokenTrajectoryChain.from_text_trajectory_chain(DS.item_to_text_chain(it), tok) for it in items]
    t2 = time.perf_counter()
    host = ILQLDataset.from_ilql_data_list([ILQLData.from_token_trajectory_chain(c) for c in chains], tok, bs)
    t3 = time.perf_counter()
    out["host"] = dict(seconds=t3 - t0, episodes_per_s=n / (t3 - t0), to_items_s=t1 - t0, tokenise_s=t2 - t1, block_s=t3 - t2)

    # ---- device path: wall clock (with the syncs a consumer pays) and HIP events per phase, median of reps
    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e
    walls, toks, blocks = [], [], []
    for _ in range(a.reps + 1):              # the first pass warms the allocator and the code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0 = ev()
        rec = loop.token_records()
        e1 = ev()
        ds = OD.ilql_data_from_records(rec, bs, tok.pad_token_id)
        e2 = ev()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        toks.append(e0.elapsed_time(e1))
        blocks.append(e1.elapsed_time(e2))
    med = lambda x: sorted(x[1:])[len(x[1:]) // 2]
    out["device"] = dict(seconds=med(walls), episodes_per_s=n / med(walls), token_records_ms=med(toks), ilql_block_ms=med(blocks))
    got = ds.to_host()
    out["device_equals_host"] = bool((got.input_ids == host.input_ids).all() and (got.should_take_action == host.should_take_action).all() and
                                     (got.rewards.view(np.uint32) == host.rewards.view(np.uint32)).all() and (got.dones == host.dones).all())
    for name, fn in (("mc", lambda: OD.mc_data_from_records(rec, a.gamma, bs, tok.pad_token_id)),
                     ("bc", lambda: OD.mask_data_from_records(rec, BlockingStrategy(Padding.RIGHT, Truncation.LEFT, a.max_length), tok.pad_token_id)),
                     ("filter_top30", lambda: OD.filter_records(rec, take_top=30))):
        ms = []
        for _ in range(a.reps + 1):
            e0 = ev()
            fn()
            e1 = ev()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        out["device"][name + "_ms"] = med(ms)
    out["speedup"] = out["device"]["episodes_per_s"] / out["host"]["episodes_per_s"]
    if a.step:
        out["ilql_step"] = _ilql_step_ms(ds, a.reps)
    loop.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
