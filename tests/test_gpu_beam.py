"""GPU tier: beam search on the device (csrc/beam.hip, the K/V reorder entries, lmrl_gym_amd/beam.py, `num_beams` of the policies) against the
float64 oracle of tests/beam_oracle.py."""
import ctypes

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
import beam_oracle as BO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NEG = BO.NEG


@pytest.fixture(scope="module")
def dev():
    from lmrl_gym_amd import _lib
    return _lib.require_gpu()


# ------------------------------------------------------------------------------------------------ 1. row kernel
@pytest.mark.parametrize("nc", [6, 32])
def test_row_topk_and_log_sum_exp(dev, nc):
    """nc = 6: the issue's shape.  nc = 32 (num_beams = 16, the widest): the per-thread lists fill 64 KB of LDS, past the default limit."""
    from lmrl_gym_amd import _lib
    L = _lib.lib()
    rows, V, ld = 6, 1000, 1024
    rng = np.random.RandomState(0)
    x = (rng.randn(rows, ld) * 3).astype(np.float32)
    x[:, V:] = 1e30                                    # beyond the vocabulary: must neither win nor enter the log-sum-exp
    top = np.sort(x[1, :V])[::-1]
    x[1, [17, 400, 900]] = top[nc - 1]                 # row 1: an exact tie across the 2K boundary (the 6th largest value four times)
    x[2, V - 1] = 50.0                                 # row 2: the maximum in the last valid column
    x[3, :8] = 40.0                                    # row 3: ties inside one 16-byte load
    x[5, 3], x[5, 1], x[5, 2] = 60.0, -0.0, 0.0        # row 5: both zeros (equal: the lower column first) among the largest of a negative row
    x[5, 4:V] = -np.abs(x[5, 4:V]) - 1.0
    x[5, 0] = -0.5
    run = np.array([0.0, -1.5, NEG, -0.25, -3.0, -7.0], dtype=np.float32)
    score = torch.zeros(rows, nc, dtype=torch.float32, device=dev)
    tok = torch.full((rows, nc), -1, dtype=torch.int32, device=dev)
    xd, rd = torch.from_numpy(x).to(dev), torch.from_numpy(run).to(dev)
    active = torch.tensor([1, 1, 1, 1, 0, 1], dtype=torch.uint8, device=dev)
    go = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    call = lambda g: _lib.check(L.lmrl_beam_row_topk(_lib.ptr(xd), ld, rows, V, nc, _lib.ptr(rd), _lib.ptr(active), g, _lib.ptr(score), _lib.ptr(tok),
                                                     _lib.stream_ptr()), "lmrl_beam_row_topk")
    call(go.data_ptr())                                # go == 0: nothing is written
    assert (tok.cpu().numpy() == -1).all()
    call(go.data_ptr() + 4)
    got_s, got_t = score.cpu().numpy().astype(np.float64), tok.cpu().numpy()
    x64 = x[:, :V].astype(np.float64)
    lse = np.log(np.exp(x64 - x64.max(1, keepdims=True)).sum(1)) + x64.max(1)
    for r in range(rows):
        if r == 4:
            assert (got_t[r] == -1).all()              # inactive row
            continue
        idx = np.argsort(-x64[r], kind="stable")[:nc]  # ties: lower column
        ref = x64[r, idx] - lse[r] + float(run[r])
        print("row", r, "max |score - ref| =", np.abs(got_s[r] - ref).max())
        assert got_t[r].tolist() == idx.tolist(), r
        assert (np.abs(got_s[r] - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all(), r
    assert (x64[1] == x64[1, got_t[1][-1]]).sum() == 4 and got_t[1][-1] == np.flatnonzero(x64[1] == x64[1, got_t[1][-1]])[0]
    assert got_t[2][0] == V - 1 and got_t[3].tolist()[:6] == [0, 1, 2, 3, 4, 5] and got_t[5].tolist()[:4] == [3, 1, 2, 0]


# ------------------------------------------------------------------------------------------------ 2. select kernel
def _dyadic(rng, lo, hi, size):
    return rng.randint(lo * 8, hi * 8, size=size) / 8.0


def _select_case(dev, seed, early, flags, fin_fixed=None, run_fixed=None, mode="random", K=3, V=16, div=False):
    """One lmrl_beam_select launch at position t = 2 on a made-up state against BO.step / BO.keep_going.  All values are multiples of 1/8 and
    length_penalty = 0, so fp32 and float64 agree exactly and ties are frequent."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.beam import BEST_RUNNING_BEAM, _State
    L = _lib.lib()
    B, cap, t, T, eos, pad, P, lpen = 3, 6, 2, 5, 2, 15, 9, 0.0
    if div:        # length_penalty = 1 with P + t = 2 and P + max_new_tokens = 4: non-unit divisors that keep every quotient exact
        T, P, lpen = 4, 0, 1.0
    rng = np.random.RandomState(seed)
    st = BO.State(B, K)
    st.run_score = -np.sort(-_dyadic(rng, -4, 0, (B, K)), axis=1) if run_fixed is None else np.array(run_fixed, dtype=np.float64)
    st.run_seq = [[[int(v) for v in rng.choice([0, 1, 3, 4, 5], size=t)] for _ in range(K)] for _ in range(B)]
    st.fin_flag = np.array(flags, dtype=bool)
    base = -np.sort(-_dyadic(rng, -6, -1, (B, K)), axis=1) if fin_fixed is None else np.array(fin_fixed, dtype=np.float64)
    st.fin_score = np.where(st.fin_flag, base, base + NEG)
    st.fin_seq = [[([int(rng.randint(3, 9))] * int(rng.randint(0, 2)) + [eos]) if st.fin_flag[b, k] else [int(v) for v in rng.randint(3, 9, size=t)]
                   for k in range(K)] for b in range(B)]
    lp = _dyadic(rng, -5, 0, (B * K, V))
    if mode == "hand":
        lp[0, eos] = 0.0                                # item 0: an eos among the top K (rank 0)
        lp[3:6] = -20.0                                 # item 1: beam 0 alone supplies the top 2K; its eos stands at rank 3 with -5, the score of a pool entry
        lp[3, [0, 1, 3, eos, 4, 5]] = [-1.0, -2.0, -3.0, -5.0, -5.5, -5.75]
    elif mode == "noeos":
        lp[:, eos] = -20.0                              # no eos among the candidates: the pools stay as they are
    new, info = BO.step(st, lp, t, P, eos, lpen, early, logprobs=True)
    # per-row candidates as lmrl_beam_row_topk hands them over
    NC = 2 * K
    flat = lp + st.run_score.reshape(-1, 1)
    order = np.argsort(-flat, axis=1, kind="stable")[:, :NC]
    cs = torch.from_numpy(np.take_along_axis(flat, order, 1).astype(np.float32)).to(dev)
    ct = torch.from_numpy(order.astype(np.int32)).to(dev)
    a, o = _State(torch, B * K, cap, dev), _State(torch, B * K, cap, dev)
    padded = lambda seqs: np.array([s + [pad] * (cap - len(s)) for r in seqs for s in r], dtype=np.int32)
    a.run_score.copy_(torch.from_numpy(st.run_score.reshape(-1).astype(np.float32)))
    a.run_hist.copy_(torch.from_numpy(padded(st.run_seq)))
    a.fin_score.copy_(torch.from_numpy(base.reshape(-1).astype(np.float32)))
    a.fin_flag.copy_(torch.from_numpy(st.fin_flag.reshape(-1).astype(np.uint8)))
    a.fin_hist.copy_(torch.from_numpy(padded(st.fin_seq)))
    o.run_hist.fill_(pad); o.fin_hist.fill_(77)
    parent, ntok, ncnt = (torch.full((B * K,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    ctl = torch.zeros(4, T + 1, dtype=torch.int32, device=dev)
    ctl[0, t] = 1
    _lib.check(L.lmrl_beam_select(ctypes.byref(a.c), ctypes.byref(o.c), _lib.ptr(cs), _lib.ptr(ct), _lib.ptr(parent), _lib.ptr(ntok), _lib.ptr(ncnt),
                                  _lib.ptr(ctl), B, K, V, cap, t, T, eos, pad, int(early), BEST_RUNNING_BEAM % K, float(P + t) ** lpen, float(P + T) ** lpen,
                                  _lib.stream_ptr()),
               "lmrl_beam_select")
    want_go = BO.keep_going(new, t + 1, T, P, lpen, early)
    assert int(ctl[0, t + 1].item()) == int(want_go), (seed, early)
    assert ncnt.cpu().tolist() == [1 if want_go else 0] * (B * K)
    assert parent.cpu().numpy().reshape(B, K).tolist() == [[b * K + int(p) for p in info[b]["parent"]] for b in range(B)]
    assert ntok.cpu().numpy().reshape(B, K).tolist() == [[int(v) for v in info[b]["tok"]] for b in range(B)]
    assert o.run_score.cpu().numpy().reshape(B, K).tolist() == new.run_score.astype(np.float32).tolist()
    assert o.run_hist.cpu().numpy()[:, : t + 1].tolist() == [s for r in new.run_seq for s in r]
    flag = o.fin_flag.cpu().numpy().reshape(B, K).astype(bool)
    assert flag.tolist() == new.fin_flag.tolist()
    eff = np.where(flag, o.fin_score.cpu().numpy().reshape(B, K).astype(np.float64), o.fin_score.cpu().numpy().reshape(B, K).astype(np.float64) + NEG)
    assert eff.tolist() == new.fin_score.tolist()
    assert o.fin_hist.cpu().numpy().tolist() == padded(new.fin_seq).tolist()
    return st, new, info, want_go


def test_select_against_the_oracle_step(dev):
    part = [[True, False, False], [True, True, False], [True, True, True]]
    # made-up cases: item 0 has an eos at rank 0; item 1's best eos (run 0 + lp -5) ties with its pool entry at -5 under length_penalty 0
    for early in (False, True):
        st, new, info, _ = _select_case(dev, 1, early, part, fin_fixed=[[-1.0, -2.0, -3.0], [-2.5, -5.0, -6.0], [-1.5, -2.5, -3.5]],
                                        run_fixed=[[-0.5, -1.0, -2.0], [0.0, -3.0, -3.5], [-0.25, -0.5, -1.0]], mode="hand")
        assert info[0]["cand_tok"][0] == 2 and 2 not in info[0]["tok"]
        assert 2 in info[1]["cand_tok"][3:] and 2 not in info[1]["cand_tok"][:3]
        assert new.fin_seq[1][1] == st.fin_seq[1][1]                   # the tie at -5: the pool entry stays ahead of the candidate
        for seed in range(2, 8):
            _select_case(dev, seed, early, part)
            _select_case(dev, seed + 100, early, [[True] * 3] * 3)      # full pools: with early stopping every candidate is penalised
            _select_case(dev, seed + 200, early, part, div=True)        # score / 2 in the pool, running score / 4 in the loop condition
        # the widest search: K = 16 (512 candidates per item, 48 merged entries)
        wide = np.random.RandomState(5).rand(3, 16) < np.array([[0.3], [0.7], [1.0]])
        _select_case(dev, 300, early, wide.tolist(), K=16, V=40)
        _select_case(dev, 301, early, wide.tolist(), K=16, V=40, div=True)
    # the loop condition is global: pools full and far ahead in items 0 and 1; item 2 alone can still improve
    high, low = [-0.125, -0.125, -0.125], [-30.0, -31.0, -32.0]
    run = [[-1.0, -2.0, -3.0]] * 3
    assert _select_case(dev, 9, False, [[True] * 3] * 3, fin_fixed=[high, high, low], run_fixed=run, mode="noeos")[3] is True
    assert _select_case(dev, 9, False, [[True] * 3] * 3, fin_fixed=[high, high, high], run_fixed=run, mode="noeos")[3] is False
    assert _select_case(dev, 9, True, [[True] * 3] * 3, fin_fixed=[high, high, low], run_fixed=run, mode="noeos")[3] is False


# ------------------------------------------------------------------------------------------------ 3. K/V reorder
def _engines(dev, cfg, sd, kind):
    from lmrl_gym_amd.gpt2 import GPT2Engine
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    return GPT2Engine(cfg, sd, dev) if kind == "bf16" else GPT2EngineF32(cfg, sd, dev, matmul=kind)


@pytest.mark.parametrize("kind", ["bf16", "f32", "bf16x3"])
def test_kv_reorder_equals_feeding_the_parents_tokens(dev, kind):
    from lmrl_gym_amd.beam import kv_reorder
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    cfg = GPT2Config(2, 2, 128, 256, 130, 96)
    eng = _engines(dev, cfg, init_hf_style_state_dict(cfg, seed=11), kind)
    R, tmax = 6, 48
    rng = np.random.RandomState(3)
    src = eng.session(2, tmax); src.reset()
    toks = np.zeros((2, 16), dtype=np.int32)
    lens = [5, 11]
    for b in range(2):
        toks[b, : lens[b]] = rng.randint(0, cfg.vocab, size=lens[b])
    src.forward(torch.from_numpy(toks.reshape(-1)).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), 16, len_bound_after=11)
    idx = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32, device=dev)
    parent = [1, 0, 0, 5, 5, 3]                       # a swap, a duplicate and an untouched source
    a, b, ref = (eng.session(R, tmax) for _ in range(3))
    for s in (a, b, ref):
        s.reset(); s.attach_prefix_from(src, idx, 11)
    steps = rng.randint(0, cfg.vocab, size=(4, R)).astype(np.int32)
    one = torch.ones(R, dtype=torch.int32, device=dev)
    for i in range(3):
        a.forward(torch.from_numpy(steps[i]).to(dev), one, 1)
        ref.forward(torch.from_numpy(steps[i][parent]).to(dev), one, 1)      # row i is fed row parent[i]'s tokens from the start
    pd = torch.tensor(parent, dtype=torch.int32, device=dev)
    go = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    b.kv.fill_(3); b.last_hidden.fill_(3); b.len.fill_(3)
    before = (b.kv.clone(), b.last_hidden.clone(), b.len.clone())
    kv_reorder(a, b, pd, go.data_ptr())               # go == 0: no byte of the destination changes
    assert torch.equal(b.kv, before[0]) and torch.equal(b.last_hidden, before[1]) and torch.equal(b.len, before[2])
    kv_reorder(a, b, pd, go.data_ptr() + 4)
    assert torch.equal(b.len, ref.len) and torch.equal(b.last_hidden, ref.last_hidden)
    b.forward(torch.from_numpy(steps[3]).to(dev), one, 1)
    ref.forward(torch.from_numpy(steps[3]).to(dev), one, 1)
    assert torch.equal(b.len, ref.len) and torch.equal(b.last_hidden, ref.last_hidden)
    assert b.len.cpu().tolist() == [9, 9, 9, 15, 15, 15]


# ------------------------------------------------------------------------------------------------ 4 / 5. end to end
E2E_SEED, E2E_EOS = 1, 7


def e2e_model(seed):
    """GPT2Config(3, 4, 256, 1024, 1000, 128), weights scaled as in test_gpu_f32_engine.py; the eos token's LM-head row is pushed along ln_f's
    bias, which raises its logit by about +3 at every position (plus a position-dependent part): hypotheses finish at different steps."""
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    cfg = GPT2Config(3, 4, 256, 1024, 1000, 128)
    sd = init_hf_style_state_dict(cfg, seed=3 + seed)
    g = torch.Generator().manual_seed(4 + seed)
    for k in sd:
        sd[k] = sd[k] * 3 + (0.1 * torch.randn(sd[k].shape, generator=g) if sd[k].dim() == 1 else 0)
    b = sd["ln_f.bias"]
    sd["wte.weight"][E2E_EOS] += 3.0 * b / float(b @ b)
    rng = np.random.RandomState(seed)
    prompts = [rng.randint(8, cfg.vocab, size=n).tolist() for n in (5, 16, 23)]
    return cfg, sd, prompts


def oracle_logits_fn(cfg, sd, prompts, K):
    from oracle import gpt2 as O

    def fn(seqs):
        return np.stack([O.forward(sd, torch.tensor([prompts[r // K] + list(s)]), cfg.n_head)[0, -1, : cfg.vocab].numpy() for r, s in enumerate(seqs)])
    return fn


@pytest.fixture(scope="module")
def e2e_reference():
    """The float64 oracle's searches, computed once for the four settings."""
    cfg, sd, prompts = e2e_model(E2E_SEED)
    fn, memo = oracle_logits_fn(cfg, sd, prompts, 4), {}

    def cached(seqs):
        key = tuple(tuple(s) for s in seqs)
        if key not in memo:
            memo[key] = fn(seqs)
        return memo[key]
    ref = {(lp, early): BO.beam_search(cached, 3, 4, 23, 8, E2E_EOS, lp, early) for lp in (1.0, 0.0) for early in (False, True)}
    return cfg, sd, prompts, ref


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("length_penalty", [1.0, 0.0])
def test_end_to_end_f32_engine_equals_the_float64_oracle(dev, e2e_reference, length_penalty, early):
    """B = 3 prompts of 5, 16 and 23 tokens, K = 4, 8 new tokens on GPT2EngineF32("f32"): sequences equal, scores within 8 x 2e-5 max(1, |ref|).
    The seed (E2E_SEED = 1) was chosen with the oracle alone: the smallest gap between adjacent candidates among the top 2K + 1 over all items,
    positions and the four settings is printed by this test and is 4.1e-3 (item 2), so no item is left out; the hypotheses finish after 1 and 2 tokens and the loop condition ends the searches after 4 or 5 positions."""
    from lmrl_gym_amd.beam import BeamSearch
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    cfg, sd, prompts, ref = e2e_reference
    seqs_ref, scores_ref, steps_ref, gaps = ref[(length_penalty, early)]
    eng = GPT2EngineF32(cfg, sd, dev, matmul="f32")
    bs = BeamSearch([eng], 3, 4, 48, length_penalty=length_penalty, early_stopping=early, eos_token_id=E2E_EOS, pad_token_id=0)
    seqs, scores = bs.run(prompts, 8)
    print("oracle gaps", gaps, "steps", steps_ref, "device steps", bs.steps, "sequences", seqs_ref, "scores", scores_ref, scores)
    left_out = [b for b in range(3) if gaps[b] < 1e-3]
    assert len(left_out) <= 1
    assert bs.steps == steps_ref or left_out
    for b in range(3):
        if b in left_out:
            continue
        assert seqs[b] == seqs_ref[b], b
        assert abs(float(scores[b]) - scores_ref[b]) <= 8 * 2e-5 * max(1.0, abs(scores_ref[b])), b


@pytest.mark.parametrize("kind,ilql", [("bf16", False), ("bf16", True), ("bf16x3", False), ("f32", True)])
def test_end_to_end_bf16_engine_replayed_by_the_oracle(dev, kind, ilql):
    """The same shapes on the bf16 GPT2Engine (and as the ILQL form: two engines, two Q heads, beta = 4).  The oracle replays the logits the search
    recorded (`trace`): every parent, token, flag and the final sequences must be the oracle's — selection, bookkeeping and reorder, without asking
    bf16 arithmetic to match float64 (a wrong reorder shows as logits of the wrong hypothesis: the trace is compared with a plain session too).
    The same replay runs on GPT2EngineF32 in "bf16x3" mode (the fused LM-head sampler's logits) and as the ILQL form in "f32" mode
    (`lmrl_value_head_logits_f32`), the two logits paths of `BeamSearch` that the float64 comparison above does not reach."""
    from lmrl_gym_amd.beam import BeamSearch
    from lmrl_gym_amd.gpt2 import GPT2Engine
    from lmrl_gym_amd.policies import heads_to_engine_layout
    from oracle import gpt2 as O
    cfg, sd, prompts = e2e_model(E2E_SEED)
    rnd = O.round_weights_to_bf16 if kind == "bf16" else (lambda x: x)          # the fp32 engine keeps its weights unrounded
    B, K, T = 3, 4, 8
    engines, heads = [_engines(dev, cfg, rnd(sd), kind)], None
    if ilql:
        _, sd_v, _ = e2e_model(E2E_SEED + 1)
        engines.append(_engines(dev, cfg, rnd(sd_v), kind))
        g = torch.Generator().manual_seed(2)
        d, V = cfg.d_model, cfg.vocab
        mk = lambda: {"dense1.kernel": torch.randn(d, d, generator=g) * 0.05, "dense1.bias": torch.randn(d, generator=g) * 0.1,
                      "dense2.kernel": torch.randn(d, V, generator=g) * 0.05, "dense2.bias": torch.randn(V, generator=g) * 0.1}
        heads = tuple(heads_to_engine_layout(mk(), cfg.vocab_padded, dev, engine=engines[0]) for _ in range(2))
    for lp, early in ((1.0, False), (0.0, True)):
        bs = BeamSearch(engines, B, K, 48, q_heads=heads, beta=4.0 if ilql else 0.0, length_penalty=lp, early_stopping=early, eos_token_id=E2E_EOS)
        trace = []
        seqs, scores = bs.run(prompts, T, trace=trace)
        live = [s for s in trace if s["go"]]
        assert len(live) == bs.steps
        checked = []

        def on_step(t, before, info, after):
            s = live[t]
            for b in range(B):
                if gaps_so_far[b] < 1e-3 or info[b]["gap"] < 1e-3:
                    gaps_so_far[b] = 0.0
                    continue
                assert s["parent"].reshape(B, K)[b].tolist() == [b * K + int(p) for p in info[b]["parent"]], (t, b)
                assert s["tok"].reshape(B, K)[b].tolist() == [int(v) for v in info[b]["tok"]], (t, b)
                assert s["fin_flag"].reshape(B, K)[b].astype(bool).tolist() == after.fin_flag[b].tolist(), (t, b)
                assert s["run_hist"].reshape(B, K, -1)[b, :, : t + 1].tolist() == after.run_seq[b], (t, b)
                checked.append((t, b))
        gaps_so_far = np.full(B, np.inf)
        seqs_ref, scores_ref, steps_ref, gaps = BO.beam_search(lambda _seqs, it=iter(live): next(it)["logits"], B, K, 23, T, E2E_EOS, lp, early, on_step=on_step)
        print(kind, "ilql", ilql, "gaps", gaps, "steps", steps_ref, bs.steps, seqs_ref, seqs)
        left_out = [b for b in range(B) if gaps[b] < 1e-3]
        assert len(left_out) <= 1
        assert steps_ref == bs.steps or left_out
        for b in range(B):
            if b not in left_out:
                assert seqs[b] == seqs_ref[b] and abs(float(scores[b]) - scores_ref[b]) <= 1e-4 * max(1.0, abs(scores_ref[b])), b
        assert len(checked) >= (B - 1) * bs.steps
        if kind == "bf16" and not ilql and lp == 1.0:
            # the logits the search saw at its last position are those of its running hypotheses in a plain session: the caches followed the beams
            ses = engines[0].session(B * K, 48); ses.reset()
            last_t = bs.steps - 1
            hyp = live[last_t - 1]["run_hist"].reshape(B * K, -1)[:, :last_t] if last_t > 0 else np.zeros((B * K, 0), dtype=np.int32)
            full = [prompts[r // K] + hyp[r].tolist() for r in range(B * K)]
            for c0 in range(0, max(len(f) for f in full), 16):
                toks = np.zeros((B * K, 16), dtype=np.int32)
                cnt = np.zeros(B * K, dtype=np.int32)
                for r, f in enumerate(full):
                    seg = f[c0: c0 + 16]
                    toks[r, : len(seg)] = seg; cnt[r] = len(seg)
                ses.forward(torch.from_numpy(toks.reshape(-1)).to(dev), torch.from_numpy(cnt).to(dev), 16, len_bound_after=min(c0 + 16, max(len(f) for f in full)))
            from lmrl_gym_amd.gpt2 import SAMPLE_WANT_LOGITS, SampleParams
            lg = torch.zeros(B * K, cfg.vocab_padded, dtype=torch.float32, device=dev)
            ses.sample(SampleParams(0.0, 0, 0, 0, 0.0, 0.0, 0, None, 0.0, 0, SAMPLE_WANT_LOGITS), logits_out=lg, want_logprob=False)
            plain = lg[:, : cfg.vocab].cpu().numpy()
            err = np.abs(plain - live[last_t]["logits"]).max()
            print("plain-session logits vs traced logits at the last position: max |diff| =", err)
            assert err <= 5e-2 * max(1.0, np.abs(plain).max())          # the bf16 engine's bound (chunked prefill vs decode steps differ in rounding)


# ------------------------------------------------------------------------------------------------ 6. policy
class CharTok:
    """Deterministic stand-in tokenizer: one token per character (as in test_gpu_policies.py)."""
    def __init__(self, vocab):
        self.vocab, self.pad_token_id, self.eos_token_id = vocab, vocab - 1, 10   # '\n'

    def encode(self, s):
        return [ord(c) % (self.vocab - 1) for c in s]

    def decode(self, ids):
        return "".join(chr(i) for i in ids)


def test_policy_num_beams(dev):
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.beam import BeamSearch
    from lmrl_gym_amd.gpt2 import GPT2Config, GPT2Engine, init_hf_style_state_dict
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    from oracle import gpt2 as O
    cfg = GPT2Config(2, 2, 128, 256, 130, 96)
    sd = O.round_weights_to_bf16({k: (v * 6 if v.dim() == 2 else v) for k, v in init_hf_style_state_dict(cfg, seed=21).items()})
    eng = GPT2Engine(cfg, sd, dev)
    tok = CharTok(cfg.vocab)
    kw = dict(max_input_length=24, max_new_tokens=6, eos_token_id=tok.eos_token_id)
    with pytest.raises(NotImplementedError, match="Beam sampling is currently not implemented."):
        GPT2PPOPolicy(eng, tok, num_beams=3, do_sample=True, **kw)
    pol = GPT2PPOPolicy(eng, tok, num_beams=3, do_sample=False, **kw)
    hists = [(E.Text("The goal is at 8, 6.\n", False),), (E.Text("a much longer observation that must be left-truncated to fit!\n", False),), (E.Text("x\n", False),),
             (E.Text("", False),)]
    done = [False, False, False, True]
    res = pol.act(hists, done)
    assert res[3] is None
    # the oracle replays the logits of the same search run directly (same kernels, same prompts, same prompt width)
    prompts = [tok.encode(tok.decode([tok.eos_token_id]) if d else E.text_history_to_str(h))[-24:] for h, d in zip(hists, done)]
    tmax = -(-(24 + 6 + 16) // 16) * 16
    bs = BeamSearch([eng], 4, 3, tmax, eos_token_id=tok.eos_token_id, pad_token_id=tok.pad_token_id)
    trace = []
    direct, _ = bs.run(prompts, 6, prompt_width=24, trace=trace)
    live = [s for s in trace if s["go"]]
    seqs_ref, _, _, gaps = BO.beam_search(lambda _s, it=iter(live): next(it)["logits"], 4, 3, 24, 6, tok.eos_token_id, 1.0, False)
    print("policy: gaps", gaps, seqs_ref, direct)
    compared = 0
    for b in range(3):
        assert res[b][:-1] == hists[b] and res[b][-1].is_action
        if gaps[b] >= 1e-3:
            special = {tok.pad_token_id}
            assert res[b][-1].text == tok.decode([t for t in seqs_ref[b] if t not in special]), b
            compared += 1
    assert compared >= 2
    # a second act with grown histories forwards only the new tokens of every prompt
    n0 = pol._beam.prefilled_tokens
    assert n0 == sum(len(p) for p in prompts)
    pol2 = GPT2PPOPolicy(eng, tok, num_beams=3, do_sample=False, max_input_length=64, max_new_tokens=6, eos_token_id=tok.eos_token_id)
    first = pol2.act([hists[0], hists[2]], [False, False])
    n1 = pol2._beam.prefilled_tokens
    second_h = [first[0] + (E.Text("ok\n", False),), first[1] + (E.Text("ok\n", False),)]
    pol2.act(second_h, [False, False])
    new_tokens = sum(len(tok.encode(E.text_history_to_str(h))) - len(tok.encode(E.text_history_to_str(h0))) for h, h0 in zip(second_h, [hists[0], hists[2]]))
    assert pol2._beam.prefilled_tokens - n1 == new_tokens, (pol2._beam.prefilled_tokens, n1, new_tokens)
    # num_beams = 1 is the existing path, untouched
    outs = []
    for extra in ({}, {"num_beams": 1}):
        p1 = GPT2PPOPolicy(eng, tok, do_sample=True, temperature=0.8, top_k=20, seed=5, **kw, **extra)
        outs.append([r[-1].text for r in p1.act(hists[:3], [False] * 3)])
        assert p1._beam is None
    assert outs[0] == outs[1]
