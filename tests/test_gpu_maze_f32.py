"""GPU tier: the Maze device rollout loop on the fp32 rollout engine (`GPT2EngineF32`, matmul "f32" and "bf16x3") — the reference's default
float32 arithmetic for Maze BC / ILQL / MC evaluation (llm_rl_scripts/maze/bc/fully_observed_bc.py:66,192: bf16_activations=False).

(a) the fp32 prompt-prefix kernels: `lmrl_attn_decode_prefixed_f32` == the gather form (`lmrl_kv_gather_f32` + `lmrl_attn_cached_f32_split3`) bit for
bit, and a float64 restatement within an fp32 bound; `lmrl_kv_gather_f32` == torch indexing; (b) the greedy device loop == the generic host text path
`interact_environment(env, GPT2ValuePolicy)` on the same fp32 engines; (c) every sampled token == the float64 oracle's argmax under the same Philox
noise; (d) indexed / copied prefix, graph / eager and per-turn prefill give identical records; (e) item windows, lanes, PPO data; (f) refusals."""
import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_maze_rollout import MergedByteTokenizer, _snapshot  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    from lmrl_gym_amd import _lib
    return _lib.require_gpu()


def _setup(dev, B, max_new, max_steps, matmul="f32", describe="describe_observation_give_position", prefix_cache=True, seed=0, boost=12.0,
           prefix_indexed=True, width="tiny", last_k=1, max_input_length=256, whole_actions_only=False, q2=False, beta=1.0):
    """`test_gpu_maze_rollout._setup` on `GPT2EngineF32`s: pi_beta, value base and the heads laid out unrounded for the engine's mode."""
    from lmrl_gym_amd.envs import maze as M
    from lmrl_gym_amd.gpt2 import GPT2Config
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    from lmrl_gym_amd.maze_rollout import MazeRolloutEngine
    from lmrl_gym_amd.policies import heads_to_engine_layout
    tok = MergedByteTokenizer()
    cfg = GPT2Config(2, 2, 128, 256, len(tok) + 3, 256) if width == "tiny" else GPT2Config(12, 12, 768, 3072, len(tok) + 3, 256)
    pi = GPT2EngineF32.random_init(cfg, seed=seed, device=dev, matmul=matmul)
    vb = GPT2EngineF32.random_init(cfg, seed=seed + 1, device=dev, matmul=matmul)
    d, V = cfg.d_model, cfg.vocab
    g = torch.Generator().manual_seed(seed + 2)
    heads = []
    for _ in range(2 if q2 else 1):
        bias = torch.full((V,), -boost)
        for i in ((256, 257, 258, 259) if whole_actions_only else (256, 257, 258, 259, 260, 261, 262, 263, 264, 10, 266, 267)):
            bias[i] = 0.0
        heads.append({"dense1.kernel": torch.randn(d, d, generator=g) * 0.05, "dense1.bias": torch.zeros(d),
                      "dense2.kernel": torch.randn(d, V, generator=g) * 0.3, "dense2.bias": bias})
    lay = [heads_to_engine_layout(h, cfg.vocab_padded, dev, engine=pi) for h in heads]
    env = M.setup_maze_env("double_t_maze", describe, "standard_reward", last_k=last_k, max_steps=max_steps)
    eng = MazeRolloutEngine(pi, tok, env, B, max_new_tokens=max_new, eos_token_id=tok.eos_token_id, prefix_cache=prefix_cache,
                            prefix_indexed=prefix_indexed, value_engine=vb, q1_head=lay[0], q2_head=lay[1] if q2 else None, beta=beta,
                            max_input_length=max_input_length)
    return eng, tok, pi, vb, lay, env, cfg, heads


def _generic(pi, vb, lay, tok, env, seeds, B, max_new, max_input_length=256):
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.maze_rollout import maze_out_str_process
    from lmrl_gym_amd.policies import GPT2ValuePolicy
    pol = GPT2ValuePolicy(pi, vb, lay[0], lay[1] if len(lay) > 1 else None, 1.0, tok, max_input_length=max_input_length, max_new_tokens=max_new,
                          do_sample=False, eos_token_id=tok.eos_token_id, out_str_process=maze_out_str_process)
    return E.interact_environment(env, pol, env_seed=seeds, bsize=B)


def _assert_same_transitions(mine, ref, B):
    assert len(mine) == len(ref) == B
    n = 0
    for b, (x, y) in enumerate(zip(mine, ref)):
        assert len(x) == len(y), (b, len(x), len(y))
        for i, (tx, ty) in enumerate(zip(x, y)):
            assert tx == ty, (b, i, tx, ty)
            n += 1
    return n


# ---------------------------------------------------------------------------------------------------------------- (a) kernels
@pytest.mark.parametrize("H,B", [(12, 37), (12, 64), (2, 130), (2, 256)])       # B * H / 4 workgroups: 111 / 192 / 65 / 128 (the XCD re-mapping needs % 8 == 0)
def test_prefixed_decode_attention_equals_the_gather_form_and_float64(dev, H, B):
    from lmrl_gym_amd import _lib
    L, p, sp = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    d = H * 64
    g = torch.Generator().manual_seed(H * 1000 + B)
    plens = [0, 1, 3, 4, 5, 31, 32, 33, 17, 40]                      # prefix lengths around the 4-position blocks and the 32-position batches
    n_rows, ptmax, tmax = len(plens), 48, 56
    pk, pv = (torch.randn(n_rows, ptmax, d, generator=g).to(dev) for _ in range(2))
    src_len = torch.tensor(plens, dtype=torch.int32, device=dev)
    idx_h = torch.randint(-1, n_rows, (B,), generator=g)
    idx_h[B // 3: B // 3 + B // 4] = 6                                 # many envs on one row
    idx_h[:len(plens)] = torch.arange(len(plens))                       # every prefix length present
    idx_h[len(plens)] = -1
    idx = idx_h.to(torch.int32).to(dev)
    gen = torch.randint(0, 6, (B,), generator=g).to(torch.int32)       # tokens generated behind the prompt so far (ragged)
    cnt_h = (torch.rand(B, generator=g) > 0.15).to(torch.int32)         # cnt = 0: finished envs
    cnt = cnt_h.to(dev)
    pn_h = torch.tensor([plens[i] if i >= 0 else 0 for i in idx_h.tolist()], dtype=torch.int32)
    lens = (pn_h + gen).to(dev)
    qkv = torch.randn(B, 3 * d, generator=g).to(dev)
    own = torch.randn(2, B, tmax, d, generator=g).to(dev)              # the env's own cache: positions [n, len) hold its generated rows
    # gather form: the prefix rows copied into the own cache (torch indexing)
    cp = own.clone()
    for b, r in enumerate(idx_h.tolist()):
        if r >= 0 and plens[r] > 0:
            cp[0, b, :plens[r]] = pk[r, :plens[r]]
            cp[1, b, :plens[r]] = pv[r, :plens[r]]
    sentinel = float("nan")
    outs = {}
    for form in ("gather", "indexed", "indexed_order"):
        kv = cp.clone() if form == "gather" else own.clone()            # indexed: positions below n hold garbage, never read
        out = torch.full((B, d), sentinel, device=dev)
        split = torch.full((B, 3 * d), -1, dtype=torch.int16, device=dev)
        if form == "gather":
            _lib.check(L.lmrl_attn_cached_f32_split3(p(qkv), p(kv[0]), p(kv[1]), p(lens), p(cnt), p(out), p(split), B, 1, H, tmax, sp), "attn")
        else:
            dlen, pn = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            order = torch.full((B,), -1, dtype=torch.int32, device=dev) if form == "indexed_order" else None
            _lib.check(L.lmrl_kv_attach_f32(n_rows, ptmax, p(src_len), None, None, p(idx), B, tmax, None, None, p(dlen), p(pn), p(order), d, sp), "attach")
            assert torch.equal(pn.cpu(), pn_h) and torch.equal(dlen.cpu(), pn_h)
            if order is not None:                                       # a permutation, grouped by prefix row (no-prefix envs last)
                o = order.cpu().numpy()
                assert sorted(o.tolist()) == list(range(B))
                key = np.where(idx_h.numpy()[o] >= 0, idx_h.numpy()[o], n_rows)
                assert (np.diff(key) >= 0).all()
            _lib.check(L.lmrl_attn_decode_prefixed_f32(p(qkv), p(kv[0]), p(kv[1]), p(lens), p(cnt), p(out), p(split), B, H, tmax, p(pk), p(pv), n_rows, ptmax,
                                                       p(idx), p(pn), p(order), sp), "prefixed")
        torch.cuda.synchronize()
        outs[form] = (out.cpu(), split.cpu(), kv.cpu())
    og, sg, kg = outs["gather"]
    for form in ("indexed", "indexed_order"):
        o, s, k = outs[form]
        assert torch.equal(o.nan_to_num(7.0), og.nan_to_num(7.0)), form
        assert torch.equal(s, sg), form
        for b in range(B):                                              # the new row appended at len in the env's OWN cache, nothing else written
            n = int(pn_h[b])
            assert torch.equal(k[:, b, n:], kg[:, b, n:]) and torch.equal(k[:, b, :n], own[:, b, :n].cpu()), (form, b)
    # float64 restatement: softmax over [prefix rows, own generated rows, the new token]
    live = cnt_h.bool()
    assert torch.isnan(og[~live]).all() and (sg[~live] == 0).all()     # finished envs: output untouched, split row zeroed
    q64, kg64 = qkv.cpu().double(), kg.double()
    for b in torch.nonzero(live).flatten().tolist():
        n = int(lens[b])
        keys = torch.cat([kg64[0, b, :n], q64[b, d:2 * d][None]])
        vals = torch.cat([kg64[1, b, :n], q64[b, 2 * d:][None]])
        for h in range(H):
            sl = slice(h * 64, h * 64 + 64)
            a = torch.softmax(keys[:, sl] @ q64[b, sl] / 8.0, 0)
            ref = a @ vals[:, sl]
            assert torch.allclose(og[b, sl].double(), ref, rtol=1e-5, atol=2e-6), (b, h, (og[b, sl].double() - ref).abs().max())
    assert int(live.sum()) > B // 2


def test_kv_gather_f32_equals_torch_indexing(dev):
    from lmrl_gym_amd import _lib
    L, p, sp = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    g = torch.Generator().manual_seed(5)
    nl, src_b, src_tmax, dst_tmax, B, d = 3, 7, 40, 36, 45, 128
    src = torch.randn(nl, 2, src_b, src_tmax, d, generator=g).to(dev)
    src_len = torch.tensor([0, 1, 3, 4, 33, 40, 17], dtype=torch.int32, device=dev)          # 40 > dst_tmax: clamped to 36
    sh, sx = torch.randn(src_b, d, generator=g).to(dev), torch.randn(src_b, d, generator=g).to(dev)
    idx_h = torch.randint(-1, src_b + 1, (B,), generator=g).to(torch.int32)                  # -1 and src_b: empty caches
    dst0 = torch.randn(nl, 2, B, dst_tmax, d, generator=g).to(dev)
    dh0, dx0 = torch.randn(B, d, generator=g).to(dev), torch.randn(B, d, generator=g).to(dev)
    dst, dh, dx, dl = dst0.clone(), dh0.clone(), dx0.clone(), torch.full((B,), -5, dtype=torch.int32, device=dev)
    _lib.check(L.lmrl_kv_gather_f32(p(src), src_b, src_tmax, p(src_len), p(sh), p(sx), p(idx_h.to(dev)), p(dst), dst_tmax, B, p(dh), p(dx), p(dl), nl, d, sp),
               "lmrl_kv_gather_f32")
    torch.cuda.synchronize()
    ref, rh, rx, rl = dst0.clone(), dh0.clone(), dx0.clone(), torch.zeros(B, dtype=torch.int32, device=dev)
    for b, r in enumerate(idx_h.tolist()):
        if 0 <= r < src_b:
            n = min(int(src_len[r]), dst_tmax)
            rl[b] = n
            if n:
                ref[:, :, b, :n] = src[:, :, r, :n]
                rh[b], rx[b] = sh[r], sx[r]
    assert torch.equal(dst, ref) and torch.equal(dh, rh) and torch.equal(dx, rx) and torch.equal(dl, rl)


# ---------------------------------------------------------------------------------------------------------------- (b) greedy == generic path
@pytest.mark.parametrize("matmul,width,B", [("f32", "tiny", 8), ("f32", "tiny", 48), ("f32", "small", 256), ("bf16x3", "tiny", 48), ("bf16x3", "small", 256)])
def test_f32_greedy_device_loop_equals_generic_text_path(dev, matmul, width, B):
    """Same fp32 engines, greedy decoding: the device loop's transitions (prefix cache, indexed rows, per-turn graph) == interact_environment with
    GPT2ValuePolicy on those engines, transition for transition.  B = 8: the fp32 sessions run without the bf16-only skinny flag."""
    from lmrl_gym_amd.gpt2 import FWD_SKINNY
    max_new, max_steps = 3, 10
    eng, tok, pi, vb, lay, env, *_ = _setup(dev, B, max_new, max_steps, matmul=matmul, boost=6.0, width=width)
    assert not eng.ses.flags & FWD_SKINNY
    seeds = [5 + 13 * i for i in range(B)]
    eng.run_episode(seeds, None, temperature=0.0, use_graph=True)
    torch.cuda.synchronize()
    mine = eng.interactions()
    n_steps = _assert_same_transitions(mine, _generic(pi, vb, lay, tok, env, seeds, B, max_new), B)
    assert n_steps >= B * 3
    kinds = {t.post_action_history[-1].text for ep in mine for t in ep}
    assert len(kinds) >= (3 if B > 16 else 2), kinds
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- (c) sampled tokens == float64 oracle
@pytest.mark.parametrize("form", ["ilql", "mc"])
@pytest.mark.parametrize("matmul,tie", [("f32", 2e-4), ("bf16x3", 3e-3)])
def test_sampled_maze_tokens_equal_the_float64_oracle(dev, matmul, tie, form):
    """Steered sampling (scripted moves, strength 3) with the ILQL (two Q heads) and MC (one) value policy: every sampled token == argmax of the
    float64 oracle's pi_beta logits + beta * min(Q1, Q2) + steer + the Philox Gumbel noise the sampler draws (counter: env row, column, step, episode
    word), except near ties; the Q heads move the argmax in a sizeable share of the draws."""
    from oracle import gpt2 as O, rl
    B, max_new, max_steps, SEED, EPISODE, BETA, STEER = 32, 3, 6, 77, 3, 3.0, 3.0
    eng, tok, pi, vb, lay, env, cfg, heads = _setup(dev, B, max_new, max_steps, matmul=matmul, boost=0.0, q2=form == "ilql", beta=BETA, seed=4)
    codes = np.random.RandomState(1).randint(0, 4, size=(eng.T, B))
    eng.set_scripted_actions(codes, strength=STEER)
    eng.run_episode([9 + 3 * i for i in range(B)], None, temperature=1.0, sample_seed=SEED, episode=EPISODE, use_graph=True, sync_every=0)
    torch.cuda.synchronize()
    tr = {k: v.cpu().numpy() for k, v in eng.traj.items()}
    st = eng.env.positions()
    R, C = eng.env.maze.shape
    acts = [tok.encode(a) for a in ("move left\n", "move right\n", "move up\n", "move down\n")]
    seqs, meta = [], []
    for b in range(B):
        gi = int(eng.goal_slot[int(st[b, 2]) * C + int(st[b, 3])])
        for t in range(int(tr["n_turns"][b])):
            r, c = int(tr["pos"][b, t]) >> 16, int(tr["pos"][b, t]) & 0xFFFF
            row = (gi * R + r) * C + c
            prompt = eng.obs_tok_h[row, :eng.obs_len_h[row]].tolist()
            gl = int(tr["gen_len"][b, t])
            seqs.append(prompt + tr["gen"][b, t, :gl].tolist())
            meta.append((b, t, len(prompt), gl))
    eng.close()
    sd_pi = _state_dict(cfg, 4)
    sd_v = _state_dict(cfg, 5)
    V = cfg.vocab
    T = max(len(s) for s in seqs)
    ids = torch.zeros(len(seqs), T, dtype=torch.int64)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = torch.tensor(s)
    logits = O.forward(sd_pi, ids, cfg.n_head)[:, :, :V]
    _, hid = O.forward(sd_v, ids, cfg.n_head, return_hidden=True)
    qs = [rl.mlp_head(hid, *(h[k] for k in ("dense1.kernel", "dense1.bias", "dense2.kernel", "dense2.bias"))) for h in heads]
    pert = rl.value_rl_logits(logits, qs[0], qs[1] if len(qs) > 1 else None, BETA).numpy()
    logits = logits.numpy()
    checked = near_tie = moved = 0
    noise_cache = {}
    for i, (b, t, n_p, gl) in enumerate(meta):
        for k in range(gl):
            key = (t, k)
            if key not in noise_cache:
                noise_cache[key] = O.gumbel_noise(B, V, SEED, k, (EPISODE << 12) + t).astype(np.float64)
            noise = noise_cache[key][b]
            a = acts[codes[t, b]]
            stk = a[k] if k < len(a) else -1
            score = pert[i, n_p + k - 1] + noise
            z_pi = logits[i, n_p + k - 1] + noise
            if stk >= 0:
                score[stk] += STEER
                z_pi[stk] += STEER
            top2 = np.partition(score, -2)[-2:]
            if top2[1] - top2[0] < tie:
                near_tie += 1
                continue
            checked += 1
            assert int(score.argmax()) == seqs[i][n_p + k], (b, t, k)
            moved += int(z_pi.argmax()) != int(score.argmax())
    print(f"{matmul} {form}: {checked} draws checked, {near_tie} near ties, Q heads moved the argmax in {moved}")
    assert checked >= 400 and near_tie <= (0.005 if matmul == "f32" else 0.03) * (checked + near_tie), (checked, near_tie)
    assert moved >= 0.2 * checked, (moved, checked)


def _state_dict(cfg, seed):
    from lmrl_gym_amd.gpt2 import init_hf_style_state_dict
    return init_hf_style_state_dict(cfg, seed)


# ---------------------------------------------------------------------------------------------------------------- (d) mode equivalence
@pytest.mark.parametrize("matmul,width,B", [("f32", "tiny", 64), ("bf16x3", "tiny", 64), ("f32", "small", 256)])
def test_f32_prefix_forms_graph_and_per_turn_prefill_give_identical_records(dev, matmul, width, B):
    """Indexed prefix eager / graph, copied prefix (graph) and per-turn prefill (eager): bit-identical records.  The per-turn prefill runs the prompt
    products at M = B * 16 rows, the prefix cache at M = n_obs * 16: for these shapes `sgemm_plan` splits K in neither (asserted below; an unsplit
    `lmrl_sgemm` is one fmaf chain over K whatever its tile), and bf16x3 at d = 128 takes no split-K product, so the K/V rows are the same bits."""
    from lmrl_gym_amd import _lib
    max_new, max_steps = 3, 6
    seeds = [31 * i + 3 for i in range(B)]
    snaps = []
    for prefix_cache, use_graph, indexed in ((True, False, True), (True, True, True), (True, True, False), (False, False, True)):
        eng, *_, cfg, _h = _setup(dev, B, max_new, max_steps, matmul=matmul, prefix_cache=prefix_cache, prefix_indexed=indexed, width=width)
        if matmul == "f32":
            d, ff = cfg.d_model, cfg.d_ff
            for m in (B * 16, eng.obs_tok_h.shape[0] * 16):
                assert all(int(_lib.lib().lmrl_sgemm_ws_bytes(m, n, k, 1)) == 0 for k, n in ((d, 3 * d), (d, d), (d, ff), (ff, d))), m
        eng.run_episode(seeds, None, temperature=0.9, sample_seed=11, episode=2, use_graph=use_graph, sync_every=0 if use_graph else 4)
        snaps.append(_snapshot(eng))
        eng.close()
    (a, pa) = snaps[0]
    for (x, px), what in zip(snaps[1:], ("graph replay", "copied prefix rows", "per-turn prefill")):
        for k in a:
            assert np.array_equal(a[k], x[k]), f"{what} differs from indexed eager launches in {k}"
        assert np.array_equal(pa, px)
    assert int(a["n_turns"].max()) == max_steps + 1


# ---------------------------------------------------------------------------------------------------------------- (e) windows, lanes, PPO data
@pytest.mark.parametrize("last_k,max_input_length,max_steps,describe,max_new", [
    (40, 1024, 7, "describe_observation_only_walls", 1), (4, 512, 6, "describe_observation_give_position", 2)])
def test_f32_history_windows_equal_the_generic_text_path(dev, last_k, max_input_length, max_steps, describe, max_new):
    B = 40
    eng, tok, pi, vb, lay, env, *_ = _setup(dev, B, max_new, max_steps, describe=describe, boost=6.0 if max_new > 1 else 30.0, last_k=last_k,
                                            max_input_length=max_input_length, whole_actions_only=max_new == 1)
    assert eng.last_k == last_k and not eng.prefix_cache
    seeds = [5 + 13 * i for i in range(B)]
    eng.run_episode(seeds, None, temperature=0.0, use_graph=False, sync_every=0)
    torch.cuda.synchronize()
    eager = eng.interactions()
    eng.run_episode(seeds, None, temperature=0.0, use_graph=True, sync_every=0)
    torch.cuda.synchronize()
    mine = eng.interactions()
    assert eng.history_flags() == 0 and mine == eager
    assert _assert_same_transitions(mine, _generic(pi, vb, lay, tok, env, seeds, B, max_new, max_input_length), B) >= B * 3
    eng.close()


def test_f32_text_env_eval_lanes_return_the_one_lane_interactions(dev):
    B, max_new, max_steps = 32, 3, 9
    out = []
    for lanes in (1, 2):
        eng, *_ = _setup(dev, B, max_new, max_steps)
        inter, summ = eng.text_env_eval(5 * B - 3, seed_generator=iter(range(400, 4000)), temperature=0.8, sample_seed=3, use_graph=True, concurrent=lanes,
                                        sync_every=4)
        assert (eng._lanes is not None and len(eng._lanes) == 2) == (lanes == 2)
        out.append((inter, summ))
        eng.close()
    assert len(out[0][0]) == 5 * B - 3 and out[0][0] == out[1][0] and out[0][1] == out[1][1]


def test_f32_maze_ppo_records_and_device_ppo_data_equal_the_host_chain_path(dev):
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.algorithms import ppo
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ppo_inference import GPT2PPOInference, text_trajectory_chains_from_transitions
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.envs import maze as M
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    from lmrl_gym_amd.maze_rollout import MazeRolloutEngine
    from lmrl_gym_amd.policies import heads_to_engine_layout
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, LinearHeadF32
    tok = ByteTokenizer()
    cfg = GPT2Config(2, 2, 128, 256, len(tok) + 3, 256)
    sd = init_hf_style_state_dict(cfg, seed=3)
    pi, vb = GPT2EngineF32(cfg, sd, dev), GPT2EngineF32.random_init(cfg, seed=4, device=dev)
    d, V = cfg.d_model, cfg.vocab
    g = torch.Generator().manual_seed(6)
    bias = torch.full((V,), -30.0)
    for ch in "movelftrighupdwn \n":
        bias[ord(ch)] = 0.0
    bias[10] = 1.5
    head = heads_to_engine_layout({"dense1.kernel": torch.randn(d, d, generator=g) * 0.05, "dense1.bias": torch.zeros(d),
                                   "dense2.kernel": torch.randn(d, V, generator=g) * 0.3, "dense2.bias": bias}, cfg.vocab_padded, dev, engine=pi)
    env = M.setup_maze_env("double_t_maze", "describe_observation_give_position", "standard_reward", last_k=1, max_steps=7)
    B = 40
    eng = MazeRolloutEngine(pi, tok, env, B, max_new_tokens=4, eos_token_id=tok.eos_token_id, value_engine=vb, q1_head=head, q2_head=None, beta=1.0)
    eng.run_episode([11 * i + 2 for i in range(B)], None, temperature=1.0, sample_seed=8, use_graph=True, sync_every=0)
    torch.cuda.synchronize()
    chains = [E.TokenTrajectoryChain.from_text_trajectory_chain(c, tok) for c in text_trajectory_chains_from_transitions(eng.interactions())]
    rec = eng.ppo_records()
    flat = [tt for c in chains for tt in c.to_list()]
    assert rec.n == len(flat) > 3 * B and rec.n_chains == B == len(chains)
    h = {k: getattr(rec, k).cpu().numpy() for k in ("tokens", "is_action", "reward", "n_tok", "done")}
    for k, tt in enumerate(flat):
        n = int(h["n_tok"][k])
        assert n == len(tt.tokens) and h["tokens"][k, :n].tolist() == tt.tokens.tolist(), k
        assert h["is_action"][k, :n].astype(bool).tolist() == tt.is_action.tolist() and np.array_equal(h["reward"][k, :n], tt.reward)
    sd2 = {kk: v + 0.02 * torch.randn(v.shape, generator=g) * v.abs().mean().clamp_min(1e-3) for kk, v in sd.items()}
    pol, init = GPT2F32(sd2, cfg.n_head, device=dev), GPT2F32(sd, cfg.n_head, device=dev)
    vh = LinearHeadF32(dict(kernel=torch.randn(d, 1, generator=g) * 0.05, bias=torch.tensor([0.2])), dev)
    inf = GPT2PPOInference(pol, vh, tok.pad_token_id, initial_policy=init)
    kw = dict(gamma=0.97, lam=0.9, kl_weight=0.05)
    max_length = rec.cap + 1
    ds, kls = eng.ppo_data(inf, max_length=max_length, bsize=64, **kw)
    datas, kls_h = inf.get_ppo_data_from_token_trajectory_chain(chains, bsize=32, max_length=max_length, **kw)
    host = ppo.PPODataset.from_ppo_data_list(datas, tok, BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, max_length))
    got = ds.to_host()
    assert (got.input_ids == host.input_ids).all() and (got.should_take_action == host.should_take_action).all()
    np.testing.assert_allclose(got.old_logprobs, host.old_logprobs, rtol=0, atol=1e-5)
    np.testing.assert_allclose(got.old_values, host.old_values, rtol=0, atol=1e-5)
    np.testing.assert_allclose(got.old_returns, host.old_returns, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got.old_advantages, host.old_advantages, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(kls.cpu().numpy(), kls_h, rtol=1e-5, atol=5e-6)
    # ---- (f) in-place weights are bf16-only: an fp32 policy is refused, pointing at set_params
    from lmrl_gym_amd import _lib
    with pytest.raises(_lib.LmrlError, match="set_params"):
        eng.load_params(pol.p)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- (f) refusals
def test_mixed_engines_and_attached_chunk_forwards_are_refused(dev):
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gpt2 import GPT2Engine
    from lmrl_gym_amd.maze_rollout import MazeRolloutEngine
    eng, tok, pi, vb, lay, env, cfg, heads = _setup(dev, 8, 2, 4)
    bf = GPT2Engine.random_init(cfg, seed=0, device=dev)
    with pytest.raises(_lib.LmrlError):            # a bf16 policy with an fp32 value base
        MazeRolloutEngine(bf, tok, env, 8, max_new_tokens=2, eos_token_id=tok.eos_token_id, value_engine=vb, q1_head=lay[0], beta=1.0)
    # a chunk forward on an attached fp32 session; reset() detaches it
    ses = pi.session(4, eng.obs_cap + 16)
    idx = torch.tensor([0, 1, -1, 0], dtype=torch.int32, device=dev)
    ses.attach_prefix_from(eng.caches[0], idx, eng.max_obs_len)
    toks, cnt = torch.zeros(4 * 16, dtype=torch.int32, device=dev), torch.ones(4, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.LmrlError):
        ses.forward(toks, cnt, 16)
    ses.forward(toks[:4], cnt, 1)                  # decode forwards are the attached session's
    ses.reset()
    ses.forward(toks, cnt, 16)
    eng.close()


def test_harness_maze_eval_runs_on_the_f32_engine(capsys):
    """`scripts/harness.py maze-eval --policy-engine f32`: the generic-path evaluation in the reference's default float32."""
    import importlib.util, json, os
    spec = importlib.util.spec_from_file_location("harness", os.path.join(os.path.dirname(__file__), "..", "scripts", "harness.py"))
    H = importlib.util.module_from_spec(spec); spec.loader.exec_module(H)
    H.main(["maze-eval", "--max-steps", "3", "--generation-bsize", "8", "--max-input-length", "160", "--max-output-length", "6", "--policy-engine", "f32"])
    me = [json.loads(l)["maze_eval"] for l in capsys.readouterr().out.splitlines() if l.startswith("{") and "maze_eval" in l]
    assert len(me) == 1 and me[0]["n"] == 26 and 0.0 <= me[0]["move_accuracy"] <= 100.0
