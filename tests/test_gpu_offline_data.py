"""GPU tier of the device offline-data build: `WordleScriptedRollouts.token_records`, `algorithms.offline_device` (csrc/offline_data.hip)
against the reference-generated fixture (tests/golden/offline_rl_data.json) and against the host path the trainers use today
(`to_items()` -> tokenizer -> `ILQLData` / `MCData` / `MaskDataset` blocking)."""
import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
from conftest import load_golden
from test_wordle_policies import G as GP, build_policy, case_vocab

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G = load_golden("offline_rl_data.json")
N_FRESH = 16384
N_DATA = 2048            # episodes of the fresh batch the blocked datasets are compared on
GAMMA = 0.99


def _host(rec):
    return {k: getattr(rec, k).cpu().numpy() for k in ("tokens", "is_action", "reward", "n_tok", "done")}


def test_token_records_equal_the_fixture_on_its_seeds():
    """(a) every fixture episode, replayed on the device loop from its seeds, then tokenised on the device: ids, flags, reward bits, n_tok, done."""
    from lmrl_gym_amd.envs import wordle_policies as P
    from lmrl_gym_amd.rollout import WordleTokenTable
    seen = 0
    for case in GP["cases"]:
        want = {e["index"]: e for e in G["episodes"] if e["case"] == case["name"]}
        if not want:
            continue
        vocab, eps = case_vocab(case), case["episodes"]
        loop = P.WordleScriptedRollouts(vocab, build_policy(case["policy"], vocab), len(eps))
        loop.run_device([ep["env_seed"] for ep in eps], [ep["policy_seed"] for ep in eps])
        rec = loop.token_records()
        h = _host(rec)
        pad = WordleTokenTable.default_gpt2().pad
        assert rec.cap == 76 and rec.n == len(eps) and rec.chain is None
        for i, e in want.items():
            n = int(h["n_tok"][i])
            assert n == len(e["tokens"]) and h["tokens"][i, :n].tolist() == e["tokens"], (case["name"], i)
            assert h["is_action"][i, :n].tolist() == e["is_action"]
            assert (h["reward"][i, :n].view(np.uint32) == np.asarray(e["reward"], np.float32).view(np.uint32)).all()
            assert bool(h["done"][i]) == e["done"]
            assert (h["tokens"][i, n:] == pad).all() and not h["is_action"][i, n:].any() and not h["reward"][i, n:].any()
            seen += 1
        part = loop.token_records(3)                                  # the first n episodes only (the last batch of a data set)
        assert part.n == 3 and (part.tokens.cpu().numpy() == h["tokens"][:3]).all()
        loop.close()
    assert seen == len(G["episodes"])


@pytest.fixture(scope="module")
def fresh():
    """16 384 fresh episodes on the 431-word list: device records, their `to_items()` and the host tokeniser's chains."""
    from lmrl_gym_amd import datasets as DS
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.envs import wordle as W, wordle_policies as P
    vocab = W.Vocabulary.builtin("wordle_official_400.txt")
    loop = P.WordleScriptedRollouts(vocab, P.RandomMixturePolicy(0.5, vocab), N_FRESH)
    rng = np.random.default_rng(20261017)
    loop.run_device(rng.integers(0, 2 ** 31 - 1, N_FRESH).tolist(), rng.integers(0, 2 ** 31 - 1, N_FRESH).tolist())
    rec = loop.token_records()
    items = loop.records().to_items()
    tok = DS.WordleTokenizer()
    chains = [E.TokenTrajectoryChain.from_text_trajectory_chain(DS.item_to_text_chain(it), tok) for it in items]
    yield dict(rec=rec, items=items, chains=chains, tok=tok, loop=loop)
    loop.close()


def test_token_records_equal_to_items_and_the_host_tokeniser_row_for_row(fresh):
    """(a) all 16 384 rows: n_tok, ids, flags, reward bits, done; every episode length occurs."""
    h = _host(fresh["rec"])
    assert len(fresh["chains"]) == N_FRESH == fresh["rec"].n
    want_n = np.array([len(c.token_trajectory.tokens) for c in fresh["chains"]])
    assert (h["n_tok"] == want_n).all() and len(set(want_n.tolist())) >= 6
    cap = fresh["rec"].cap
    tok_w = np.full((N_FRESH, cap), fresh["tok"].pad_token_id, np.int32)
    ia_w, rw_w = np.zeros((N_FRESH, cap), np.uint8), np.zeros((N_FRESH, cap), np.float32)
    for i, c in enumerate(fresh["chains"]):
        tt = c.token_trajectory
        n = len(tt.tokens)
        tok_w[i, :n], ia_w[i, :n], rw_w[i, :n] = tt.tokens, tt.is_action, tt.reward
    assert (h["tokens"] == tok_w).all() and (h["is_action"] == ia_w).all()
    assert (h["reward"].view(np.uint32) == rw_w.view(np.uint32)).all()
    assert (h["done"].astype(bool) == np.array([bool(c.token_trajectory.done) for c in fresh["chains"]])).all()


def _sub(rec, n):
    from lmrl_gym_amd.algorithms.ppo_device import PPORecords
    return PPORecords(rec.tokens[:n], rec.is_action[:n], rec.reward[:n], rec.n_tok[:n], rec.done[:n])


@pytest.mark.parametrize("trunc", ["RIGHT", "LEFT"])
@pytest.mark.parametrize("T", [40, 128])
def test_device_datasets_equal_the_host_datasets(fresh, trunc, T):
    """(b) ILQL / MC / BC datasets built on the device == the host datasets of the same episodes: ids, masks, rewards, dones bit for bit; MC
    returns within the bound that pins `lmrl_rtg` to the reference's numpy output (tests/test_gpu_losses_pinned.py: rtol = 3e-5,
    atol = 3e-5 * max(1, |ref|max)).  T = 40 cuts most episodes of four turns or more, inside actions and observations; T = 128 cuts none."""
    from lmrl_gym_amd.algorithms import offline_device as OD
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ilql import ILQLData, ILQLDataset
    from lmrl_gym_amd.algorithms.mc_returns import MCData
    from lmrl_gym_amd.datasets import MaskDataset
    bs = BlockingStrategy(Padding.RIGHT, getattr(Truncation, trunc), T)
    rec, chains, tok = _sub(fresh["rec"], N_DATA), fresh["chains"][:N_DATA], fresh["tok"]
    pad = tok.pad_token_id
    n_cut = sum(len(c.token_trajectory.tokens) > T for c in chains)
    assert (n_cut > N_DATA // 4) if T == 40 else n_cut == 0
    # ILQL
    host = ILQLDataset.from_ilql_data_list([ILQLData.from_token_trajectory_chain(c) for c in chains], tok, bs)
    dev = OD.ilql_data_from_records(rec, bs, pad)
    got = dev.to_host()
    assert isinstance(got, ILQLDataset) and got.next_token_ids is None and got.next_dones is None
    assert got.input_ids.dtype == np.int32 and (got.input_ids == host.input_ids).all()
    assert got.should_take_action.dtype == np.bool_ and (got.should_take_action == host.should_take_action).all()
    assert (got.rewards.view(np.uint32) == host.rewards.view(np.uint32)).all()
    assert got.dones.dtype == np.bool_ and (got.dones == host.dones).all() and host.dones.any()
    assert (dev.lengths.cpu().numpy() == np.minimum([len(c.token_trajectory.tokens) for c in chains], T)).all()
    # MC
    mch = MCData.block([MCData.from_token_trajectory_chain(c, GAMMA) for c in chains[:512]], bs, tok)
    mcd = OD.mc_data_from_records(_sub(rec, 512), GAMMA, bs, pad).to_host()
    assert (mcd["input_ids"] == mch["input_ids"]).all() and (mcd["should_take_action"] == mch["should_take_action"]).all()
    diff = np.abs(mcd["returns"] - mch["returns"])
    print(f"MC returns T={T} {trunc}: max abs diff {diff.max():.3e}, |ref|max {np.abs(mch['returns']).max():.4f}")
    np.testing.assert_allclose(mcd["returns"], mch["returns"], rtol=3e-5, atol=3e-5 * max(1.0, float(np.abs(mch["returns"]).max())))
    assert (mcd["returns"][~mch["should_take_action"]] == 0).all()
    # BC
    mdh = MaskDataset.blocked_from_str_segments([it["sequence"] for it in fresh["items"][:N_DATA]], tok, bs)
    mdd = OD.mask_data_from_records(rec, bs, pad).to_host()
    assert isinstance(mdd, MaskDataset) and (mdd.input_ids == mdh.input_ids).all()
    assert mdd.input_training_mask.dtype == np.float32 and (mdd.input_training_mask == mdh.input_training_mask).all()


def test_unbuilt_strategies_and_chains_raise(fresh):
    from lmrl_gym_amd.algorithms import offline_device as OD
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ppo_device import PPORecords
    rec = _sub(fresh["rec"], 8)
    with pytest.raises(ValueError):
        OD.ilql_data_from_records(rec, BlockingStrategy(Padding.LEFT, Truncation.RIGHT, 64), 0)
    z = torch.zeros(8, dtype=torch.int32, device=rec.tokens.device)
    chained = PPORecords(rec.tokens, rec.is_action, rec.reward, rec.n_tok, rec.done[:1], chain=z, pos=z, last=z.to(torch.uint8), n_chains=1)
    with pytest.raises(ValueError):
        OD.mc_data_from_records(chained, GAMMA, BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, 64), 0)


def test_batches_filter_and_concat(fresh):
    """Batches are rows of the dataset with the masks of their lengths; `filter_records` keeps what the host rules keep from the host's own
    reward sums; a filtered build equals the rows of the full one; `concat` stacks parts."""
    from lmrl_gym_amd.algorithms import bc, offline_device as OD
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation, initialize_attn_mask_pos_ids
    rec, tok = _sub(fresh["rec"], N_DATA), fresh["tok"]
    items = fresh["items"][:N_DATA]
    bs = BlockingStrategy(Padding.RIGHT, Truncation.LEFT, 128)
    ds = OD.ilql_data_from_records(rec, bs, tok.pad_token_id)
    full = ds.to_host()
    assert ds.longest == int(rec.n_tok.max().item()) and ds.trimmed_width() == 128 and ds.trimmed_width(8) == -(-ds.longest // 8) * 8
    idx = np.array([5, 0, 2047, 77, 5], dtype=np.int64)
    w = ds.trimmed_width(8)
    b = ds.batch(idx, width=w)
    assert set(b) == {"input_ids", "should_take_action", "rewards", "dones", "next_token_ids", "next_dones", "attention_mask", "position_ids"}
    assert b["next_token_ids"] is None and b["input_ids"].is_cuda
    assert (b["input_ids"].cpu().numpy() == full.input_ids[idx, :w]).all() and (b["rewards"].cpu().numpy() == full.rewards[idx, :w - 1]).all()
    assert (b["should_take_action"].cpu().numpy().astype(bool) == full.should_take_action[idx, :w - 1]).all()
    assert (b["dones"].cpu().numpy().astype(bool) == full.dones[idx]).all()
    am, pos = initialize_attn_mask_pos_ids(full.input_ids[idx, :w], tok.pad_token_id)
    assert (b["attention_mask"].cpu().numpy() == am).all() and (b["position_ids"].cpu().numpy() == pos).all()
    with pytest.raises(ValueError):
        ds.batch(idx, width=ds.longest - 1)
    assert sum(x["input_ids"].shape[0] for x in ds.batches(np.random.default_rng(0), 500)) == 2000
    # the filter: scores == the host's sums; kept rows == the host rules on them
    scores = OD.record_returns(rec).cpu().numpy()
    host_scores = np.array([sum(it["reward"]) for it in items])
    assert scores.dtype == np.float32 and (scores == host_scores.astype(np.float32)).all() and len(set(host_scores.tolist())) >= 6
    order = list(range(N_DATA))
    for kw, want in ((dict(take_top=30), bc.filter_items(lambda i: host_scores[i], order, take_top=30)),
                     (dict(threshold=-3.0), bc.filter_items(lambda i: host_scores[i], order, threshold=-3.0)),
                     (dict(top_fraction=0.3), sorted(order, key=lambda i: host_scores[i], reverse=True)[: int(N_DATA * 0.3)])):
        keep = OD.filter_records(rec, **kw)
        assert keep.rows.is_cuda and keep.rows.dtype == torch.int32 and keep.rows.cpu().numpy().tolist() == want == keep.rows_host.tolist()
        assert 0 < len(want) < N_DATA and len(keep) == len(want)
        md = OD.mask_data_from_records(rec, bs, tok.pad_token_id, keep=keep)
        mfull = OD.mask_data_from_records(rec, bs, tok.pad_token_id).to_host()
        assert (md.to_host().input_ids == mfull.input_ids[want]).all() and (md.to_host().input_training_mask == mfull.input_training_mask[want]).all()
        assert (md.batch(np.arange(4))["is_action"].cpu().numpy() == mfull.input_training_mask[want[:4]]).all()
    # concat
    parts = [OD.ilql_data_from_records(_sub(rec, 100), bs, tok.pad_token_id), OD.ilql_data_from_records(_sub(rec, 40), bs, tok.pad_token_id)]
    cat = OD.DeviceILQLDataset.concat(parts)
    assert len(cat) == 140 and (cat.to_host().input_ids == np.concatenate([full.input_ids[:100], full.input_ids[:40]])).all()
    assert cat.longest == max(p.longest for p in parts) and (cat.lengths.cpu().numpy()[100:] == ds.lengths.cpu().numpy()[:40]).all()


def test_streamed_device_dataset_equals_the_jsonl_path():
    """`wordle_offline_dataset_device` (three launch sequences, concatenated) == `generate_wordle_dataset_device` items on the same seed through
    the host builders, for the three kinds."""
    from lmrl_gym_amd import datasets as DS
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ilql import ILQLData, ILQLDataset
    from lmrl_gym_amd.algorithms.mc_returns import MCData
    from lmrl_gym_amd.envs import wordle as W, wordle_policies as P
    vocab = W.Vocabulary.builtin("wordle_official_400.txt")
    pol = lambda: P.RandomMixturePolicy(0.7, vocab)
    tok = DS.WordleTokenizer()
    items = DS.generate_wordle_dataset_device(vocab, 300, pol(), seed=11, bsize=128)
    chains = [E.TokenTrajectoryChain.from_text_trajectory_chain(DS.item_to_text_chain(it), tok) for it in items]
    bs = BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, 64)
    il = DS.wordle_offline_dataset_device(vocab, 300, pol(), kind="ilql", seed=11, bsize=128, max_length=64).to_host()
    host = ILQLDataset.from_ilql_data_list([ILQLData.from_token_trajectory_chain(c) for c in chains], tok, bs)
    assert il.input_ids.shape == (300, 64) and (il.input_ids == host.input_ids).all() and (il.should_take_action == host.should_take_action).all()
    assert (il.rewards.view(np.uint32) == host.rewards.view(np.uint32)).all() and (il.dones == host.dones).all()
    mc = DS.wordle_offline_dataset_device(vocab, 300, pol(), kind="mc", seed=11, bsize=128, max_length=64, gamma=GAMMA).to_host()
    mch = MCData.block([MCData.from_token_trajectory_chain(c, GAMMA) for c in chains], bs, tok)
    assert (mc["input_ids"] == mch["input_ids"]).all()
    np.testing.assert_allclose(mc["returns"], mch["returns"], rtol=3e-5, atol=3e-5 * max(1.0, float(np.abs(mch["returns"]).max())))
    bl = BlockingStrategy(Padding.RIGHT, Truncation.LEFT, 64)
    md = DS.wordle_offline_dataset_device(vocab, 300, pol(), kind="bc", seed=11, bsize=128, max_length=64, truncation=Truncation.LEFT).to_host()
    mdh = DS.MaskDataset.blocked_from_str_segments([it["sequence"] for it in items], tok, bl)
    assert (md.input_ids == mdh.input_ids).all() and (md.input_training_mask == mdh.input_training_mask).all()
    with pytest.raises(ValueError):
        DS.wordle_offline_dataset_device(vocab, 8, pol(), kind="ppo")


def test_chain_records_of_the_maze_loop_equal_the_host_ilql_items():
    """(b, chains) `MazeRolloutEngine.ppo_records()` (one trajectory per transition, chained per episode) -> `ilql_data_from_records` ==
    `ILQLData.from_token_trajectory_chain` on the host chains of the same episodes, link for link, under both truncations; a chain's last
    link (next None in the reference) has an all-padding next row and next_done = True."""
    from lmrl_gym_amd import _lib, environment as E
    from lmrl_gym_amd.algorithms import offline_device as OD
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ilql import ILQLData
    from lmrl_gym_amd.algorithms.ppo_inference import text_trajectory_chains_from_transitions
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.envs import maze as M
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine, init_hf_style_state_dict
    from lmrl_gym_amd.maze_rollout import MazeRolloutEngine
    from lmrl_gym_amd.policies import heads_to_engine_layout
    dev = _lib.require_gpu()
    tok = ByteTokenizer()
    cfg = GPT2Config(2, 2, 128, 256, len(tok) + 3, 256)
    pi, vb = GPT2Engine(cfg, init_hf_style_state_dict(cfg, seed=3), dev), GPT2Engine.random_init(cfg, seed=4, device=dev)
    d, V = cfg.d_model, cfg.vocab
    g = torch.Generator().manual_seed(6)
    bias = torch.full((V,), -30.0)
    for ch in "movelftrighupdwn \n":
        bias[ord(ch)] = 0.0
    bias[10] = 1.5
    head = heads_to_engine_layout({"dense1.kernel": torch.randn(d, d, generator=g) * 0.05, "dense1.bias": torch.zeros(d),
                                   "dense2.kernel": torch.randn(d, V, generator=g) * 0.3, "dense2.bias": bias}, cfg.vocab_padded, dev)
    env = M.setup_maze_env("double_t_maze", "describe_observation_give_position", "standard_reward", last_k=1, max_steps=7)
    B = 40
    eng = MazeRolloutEngine(pi, tok, env, B, max_new_tokens=4, eos_token_id=tok.eos_token_id, value_engine=vb, q1_head=head, q2_head=None, beta=1.0)
    eng.run_episode([11 * i + 2 for i in range(B)], None, temperature=1.0, sample_seed=8, use_graph=False, sync_every=0)
    torch.cuda.synchronize()
    chains = [E.TokenTrajectoryChain.from_text_trajectory_chain(c, tok) for c in text_trajectory_chains_from_transitions(eng.interactions())]
    rec = eng.ppo_records()
    links = []
    for c in chains:
        cur = c
        while cur is not None:
            links.append(cur)
            cur = cur.next
    assert rec.n == len(links) > 3 * B and rec.chain is not None
    longest = max(len(l.token_trajectory.tokens) for l in links)
    with_next = [i for i, l in enumerate(links) if l.next is not None]
    ends = [i for i, l in enumerate(links) if l.next is None]
    assert len(ends) == B and len(with_next) > 2 * B
    for trunc, T in ((Truncation.RIGHT, longest + 3), (Truncation.RIGHT, longest // 2), (Truncation.LEFT, longest // 2)):
        bs = BlockingStrategy(Padding.RIGHT, trunc, T)
        got = OD.ilql_data_from_records(rec, bs, tok.pad_token_id).to_host()
        host = ILQLData.block([ILQLData.from_token_trajectory_chain(links[i]) for i in with_next], bs, tok)
        assert (got.input_ids[with_next] == host["input_ids"]).all() and (got.should_take_action[with_next] == host["should_take_action"]).all()
        assert (got.rewards[with_next].view(np.uint32) == host["rewards"].view(np.uint32)).all()
        assert (got.dones[with_next] == host["dones"]).all() and not host["dones"].any()
        assert (got.next_token_ids[with_next] == host["next_token_ids"]).all() and (got.next_dones[with_next] == host["next_dones"]).all()
        assert (got.next_token_ids[ends] == tok.pad_token_id).all() and got.next_dones[ends].all()
        assert (got.dones[ends] == np.array([bool(links[i].token_trajectory.done) for i in ends])).all()
        for i in ends[:5]:
            n = min(len(links[i].token_trajectory.tokens), T)
            src = links[i].token_trajectory.tokens
            assert got.input_ids[i, :n].tolist() == (src[:n] if trunc == Truncation.RIGHT else src[len(src) - n:]).tolist()
    # the chain filter keeps every row of a kept chain
    keep = OD.filter_records(rec, top_fraction=0.25).rows.cpu().numpy()
    scores = OD.record_returns(rec).cpu().numpy()
    host_scores = np.array([sum(float(tt.reward.sum()) for tt in c.to_list()) for c in chains], dtype=np.float32)
    assert np.allclose(scores, host_scores, rtol=0, atol=1e-6)
    kept_chains = sorted(range(B), key=lambda i: scores[i], reverse=True)[:10]
    chain_h = rec.chain.cpu().numpy()
    assert keep.tolist() == [int(r) for c in kept_chains for r in np.flatnonzero(chain_h == c)]


# ------------------------------------------------------------------------------------------------ (c) train steps on device batches
def _flat(d, pre=""):
    out = {}
    for k, x in d.items():
        out.update(_flat(x, pre + k + ".") if isinstance(x, dict) else {pre + k: float(x)})
    return out


def _toy(dev, matmul):
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, MLPHeadF32
    cfg = GPT2Config(2, 2, 128, 512, 50258, 128)          # the Wordle table's pad id (50257) is the last id of the vocabulary
    sd = init_hf_style_state_dict(cfg, seed=9)
    g = torch.Generator().manual_seed(13)
    d = cfg.d_model
    mk = lambda out: {"dense1.kernel": torch.randn(d, d, generator=g) * 0.1, "dense1.bias": torch.randn(d, generator=g) * 0.1,
                      "dense2.kernel": torch.randn(d, out, generator=g) * 0.1, "dense2.bias": torch.full((out,), -0.4)}
    base = lambda scale=1.0: GPT2F32({k: v.clone() * scale for k, v in sd.items()}, cfg.n_head, device=dev, matmul=matmul)
    head = lambda out: MLPHeadF32(mk(out), dev, matmul=matmul)
    return cfg, base, head


def _same_step(outs):
    (l0, g0, grads0, p0), (l1, g1, grads1, p1) = outs
    assert l0 == l1 and np.isfinite(l0)
    f0, f1 = _flat(g0), _flat(g1)
    assert f0.keys() == f1.keys() and len(f0) >= 1
    for k in f0:
        assert f0[k] == f1[k] or (np.isnan(f0[k]) and np.isnan(f1[k])), k
    assert len(grads0) == len(grads1) and len(p0) == len(p1)
    for a, b in zip(grads0 + p0, grads1 + p1):
        assert torch.equal(a, b)
    assert sum(float(a.abs().sum()) for a in grads0) > 0


def _grad_list(last_grads):
    gs = last_grads if isinstance(last_grads, (tuple, list)) else (last_grads,)
    return [v.detach().clone() for g in gs for _, v in sorted(g.items())]


def _params(*models):
    return [v.detach().clone() for m in models for _, v in sorted(m.p.items())]


@pytest.mark.parametrize("matmul", ["f32", "bf16"])
@pytest.mark.parametrize("algo", ["ilql", "ilql_chain", "mc", "bc"])
def test_train_step_on_a_device_batch_equals_the_numpy_batch(fresh, algo, matmul):
    """(c) `step(**device batch)` == `step(**numpy batch)` on the same rows: loss, every log, the gradients and the updated parameters, bit for
    bit, in f32 and in the bf16-matmul mode at toy width."""
    from lmrl_gym_amd import _lib, environment as E
    from lmrl_gym_amd.algorithms import bc, ilql, mc_returns as mc, offline_device as OD
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ppo_device import PPORecords
    dev = _lib.require_gpu()
    tok = fresh["tok"]
    pad = tok.pad_token_id
    bs = BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, 80)
    rec = _sub(fresh["rec"], 256)
    index = np.random.RandomState(1).permutation(256)[:24]
    if algo == "ilql":
        ds = OD.ilql_data_from_records(rec, bs, pad)
        h = ds.to_host()[index]
        host = {k: v for k, v in h.items() if v is not None}
    elif algo == "ilql_chain":
        arr = lambda x, dt: np.asarray(x, dtype=dt)
        chains = []
        for c in G["chains"] * 3:
            nxt = None
            for l in reversed(c["links"]):
                nxt = E.TokenTrajectoryChain(E.TokenTrajectory(arr(l["tokens"], np.int32), arr(l["is_action"], np.bool_), arr(l["reward"], np.float32),
                                                               np.asarray(l["done"])), nxt)
            chains.append(nxt)
        ds = OD.ilql_data_from_records(PPORecords.from_token_trajectory_chains(chains, device=dev), BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, 24), pad)
        index = np.random.RandomState(2).permutation(len(ds))[:16]
        host = ds.to_host()[index]
        assert host["next_token_ids"] is not None and host["next_dones"].any() and not host["next_dones"].all()
    elif algo == "mc":
        ds = OD.mc_data_from_records(rec, GAMMA, bs, pad)
        hd = ds.to_host()
        host = {k: v[index] for k, v in hd.items()}
    else:
        ds = OD.mask_data_from_records(rec, BlockingStrategy(Padding.RIGHT, Truncation.LEFT, 80), pad)
        hd = ds.to_host()
        host = dict(input_ids=hd.input_ids[index], is_action=hd.input_training_mask[index])
    batch_d = ds.batch(index)
    for k, v in host.items():
        assert np.array_equal(batch_d[k].cpu().numpy().astype(v.dtype), v), k
    assert all(x is None or x.is_cuda for x in batch_d.values())
    outs = []
    for batch in (host, batch_d):
        cfg, base, head = _toy(dev, matmul)
        V = cfg.vocab
        if algo.startswith("ilql"):
            b = base()
            tr = ilql.GPT2ILQLTrain(b, head(V), head(V), head(1), pad, dict(gamma=0.99, tau=0.7, cql_weight=0.01), target_base=base(1.01), lr=1e-3)
            models = (b, tr.q1, tr.q2, tr.v, tr.q1_target, tr.q2_target)
        elif algo == "mc":
            b = base()
            tr = mc.GPT2MCTrain(b, head(V), pad, dict(cql_weight=0.05), lr=1e-3)
            models = (b, tr.q_head)
        else:
            b = base()
            tr = bc.GPT2BCTrain(b, pad, non_action_weight=0.3, lr=1e-3)
            models = (b,)
        _, loss, logs = tr.step(**batch)
        torch.cuda.synchronize()
        outs.append((loss, logs, _grad_list(tr.last_grads), _params(*models)))
    _same_step(outs)


def test_keep_lists_are_validated(fresh):
    from lmrl_gym_amd.algorithms import offline_device as OD
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ppo_device import PPORecords
    rec = _sub(fresh["rec"], 8)
    bs = BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, 80)
    for bad in ([0, 8], [-1, 2], []):
        with pytest.raises(ValueError):
            OD.mask_data_from_records(rec, bs, 0, keep=bad)
    ch = torch.tensor([0, 0, 1, 1, 1, 2, 2, 3], dtype=torch.int32, device=rec.tokens.device)
    last = torch.tensor([0, 1, 0, 0, 1, 0, 1, 1], dtype=torch.uint8, device=rec.tokens.device)
    chained = PPORecords(rec.tokens, rec.is_action, rec.reward, rec.n_tok, rec.done[:4], chain=ch, pos=torch.zeros_like(ch), last=last, n_chains=4)
    with pytest.raises(ValueError):
        OD.ilql_data_from_records(chained, bs, 0, keep=[2, 3])                  # chain 1 without its last trajectory
    assert len(OD.ilql_data_from_records(chained, bs, 0, keep=[2, 3, 4, 7])) == 4


# ------------------------------------------------------------------------------------------------ (d) the harness on device data
def _harness():
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("harness", os.path.join(os.path.dirname(__file__), "..", "scripts", "harness.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    return H


def _logged(capsys, tag):
    import json
    out = []
    for line in capsys.readouterr().out.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            if tag in d:
                out.append(d[tag])
    return out


def test_harness_runs_on_device_data_at_toy_scale(capsys):
    """(d) `harness.py filtered-bc --device-rollouts 1 --device-data 1` (records -> filter -> DeviceMaskDataset -> steps -> load_params in place, two
    rounds on one engine) and `harness.py ilql --device-data 1` complete; the resident filtered-BC round keeps the episodes the host path keeps on
    the same seeds (first round: same weights, same sampler key)."""
    H = _harness()
    common = ["filtered-bc", "--n-rollouts", "10", "--rollout-bsize", "4", "--filter-percengage", "0.5", "--train-bsize", "2", "--max-input-length", "96",
              "--max-output-length", "6", "--device-rollouts", "1"]
    H.main(common + ["--n-rounds", "1", "--max-steps", "1"])
    host = _logged(capsys, "data_collection")
    H.main(common + ["--n-rounds", "2", "--max-steps", "3", "--device-data", "1"])
    out = capsys.readouterr().out
    import json
    lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    res = [d["data_collection"] for d in lines if "data_collection" in d]
    assert len(host) == 1 and len(res) == 2 and res[0]["device_resident"]
    assert res[0]["kept"] == 5 and res[0]["kept_episodes"] == host[0]["kept_episodes"] and res[0]["reward_cutoff"] == host[0]["reward_cutoff"]
    assert res[0]["env_interaction"]["reward"]["mean"] == pytest.approx(host[0]["env_interaction"]["reward"]["mean"], abs=1e-6)
    steps = [d["train"] for d in lines if "train" in d]
    assert [s["step"] for s in steps] == [1, 2, 3] and {s["round"] for s in steps} == {0, 1} and all(np.isfinite(s["loss"]) for s in steps)
    assert any("eval" in d for d in lines)
    with pytest.raises(SystemExit):
        H.main(["filtered-bc", "--device-data", "1", "--n-rollouts", "4", "--rollout-bsize", "4"])
    H.main(["ilql", "--device-data", "1", "--n-data", "48", "--prob-smart", "0.6", "--data-bsize", "32", "--epochs", "1", "--max-steps", "2", "--train-bsize", "8",
            "--max-length", "80", "--log-every", "1", "--policy-n-rollouts", "4", "--policy-bsize", "4", "--beta", "4", "--device-rollouts", "1"])
    out = capsys.readouterr().out
    lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert [d["device_data"]["episodes"] for d in lines if "device_data" in d] == [48]
    tr = [d["train"] for d in lines if "train" in d]
    assert [t["step"] for t in tr] == [1, 2] and all(np.isfinite(t["loss"]) for t in tr) and any("eval" in d for d in lines)
    with pytest.raises(SystemExit):
        H.main(["ilql", "--epochs", "1"])


def test_replayed_graph_runs_on_the_weights_loaded_in_place(fresh):
    """(d) `record_rollouts` on the graph path, BC steps on the kept rows, `load_params` into the same engine, then the SAME captured graph is
    replayed: it runs on the new weights (the engine's buffers hold them) and yields a full set of records again."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.algorithms import bc, offline_device as OD
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.envs import wordle as W
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine, init_hf_style_state_dict
    from lmrl_gym_amd.rollout import WordleRolloutEngine
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32
    dev = _lib.require_gpu()
    cfg = GPT2Config(2, 2, 128, 512, 50257, 128)
    sd = init_hf_style_state_dict(cfg, seed=5)
    B = 16
    ro = WordleRolloutEngine(GPT2Engine(cfg, sd, dev), W.Vocabulary.builtin("wordle_official_400.txt"), B, max_new_tokens=6, bad_word_reward=-10.0)
    rec, summary = ro.record_rollouts(2 * B + 5, seed_generator=iter(range(100, 10 ** 6)), sample_seed=4, use_graph=True)
    assert rec.n == 2 * B + 5 and rec.chain is None and summary["length"]["max"] <= 6 and int(rec.n_tok.min().item()) > 4
    graph_key = ro._eval_graph_key
    keep = OD.filter_records(rec, top_fraction=0.5)
    ds = OD.mask_data_from_records(rec, BlockingStrategy(Padding.RIGHT, Truncation.LEFT, 128), ro.tokens.pad, keep=keep)
    assert len(ds) == (2 * B + 5) // 2
    model = GPT2F32(sd, cfg.n_head, device=dev)
    tr = bc.GPT2BCTrain(model, ro.tokens.pad, lr=1e-2)
    for batch in ds.batches(np.random.default_rng(0), 6, width=ds.trimmed_width(8)):
        _, loss, _ = tr.step(**batch)
        assert np.isfinite(loss)
    before = ro.eng.layers[0][2].clone()
    ro.load_params(model.p)
    torch.cuda.synchronize()
    assert not torch.equal(before, ro.eng.layers[0][2])
    assert torch.equal(ro.eng.layers[0][2], model.p["h.0.attn.c_attn.weight"].t().to(torch.bfloat16))
    rec2, _ = ro.record_rollouts(B, seed_generator=iter(range(100, 10 ** 6)), sample_seed=4, use_graph=True)
    assert ro._eval_graph_key == graph_key and rec2.n == B and int(rec2.n_tok.min().item()) > 4
    ro.close()
