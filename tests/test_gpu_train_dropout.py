"""GPU tier: dropout in the GPT-2 train steps (csrc/dropout.h, dropout.hip, the DROP sweeps of flash_attn_train.hip).

Model: 2 layers, d = 128, 2 heads (head width 64: the flash kernels are taken), d_ff = 512, vocab 211; B = 3, T = 80 (two 64-key tiles, the
second ragged), one row right-padded to length 50; rates embd 0.10 / attn 0.25 / resid 0.15 (distinct: a swapped site shows).
Oracle: a float64 torch-CPU GPT-2 with autograd written here, its keep masks from the documented rule — fold_in(key, site), the words of
jax.random.bits, uniform < 1 - p — restated on numpy uint32 arrays and anchored to `jax_prng.threefry2x32` / `jax_prng.random_bits`.
Nothing of the oracle comes from the device.
Bounds (those of tests/test_gpu_train_width.py for this arithmetic): values, losses and log entries 1e-4 relative; gradients 3e-4 of the
tensor's largest entry.  bf16-matmul mode against our fp32 step with the same key (identical masks): those of tests/test_gpu_train_bf16.py —
loss 2e-2 relative, every gradient tensor relative L2 <= 0.10 and cosine >= 0.995; a tensor beyond them is measured against the SAME pair of
steps without dropout and may reach 1.5 x that no-dropout figure (see `test_bf16_matmul_ilql_step_with_dropout`).
"""
import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
from lmrl_gym_amd import jax_prng

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, NH, D, DFF, NL = 211, 2, 128, 512, 2
B, T, PAD = 3, 80, 210
RATES = dict(embd_pdrop=0.10, attn_pdrop=0.25, resid_pdrop=0.15)
KEY = jax_prng.split(jax_prng.prng_key(1234))[1]
KEY2 = jax_prng.split(jax_prng.prng_key(99))[1]


@pytest.fixture(scope="module")
def dev():
    from lmrl_gym_amd import _lib
    return _lib.require_gpu()


# ------------------------------------------------------------------------------------------------ the mask rule, restated
def _threefry(key, c0, c1):
    """Threefry-2x32, 20 rounds, on uint32 arrays (jax_prng.threefry2x32 elementwise)"""
    rotl = lambda x, r: (x << np.uint32(r)) | (x >> np.uint32(32 - r))
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    ks = (k0, k1, k0 ^ k1 ^ np.uint32(0x1BD11BDA))
    x0, x1 = c0 + ks[0], c1 + ks[1]
    for g in range(5):
        for r in ((13, 15, 26, 6), (17, 29, 16, 24))[g % 2]:
            x0 = x0 + x1
            x1 = rotl(x1, r) ^ x0
        x0 = x0 + ks[(g + 1) % 3]
        x1 = x1 + ks[(g + 2) % 3] + np.uint32(g + 1)
    return x0, x1


_MASKS = {}


def keep_mask(key, site, shape, p):
    """float64 tensor `shape` of mask / (1 - p): keep[i] = bitcast((bits[i] >> 9) | 0x3F800000) - 1.0f < 1 - p (fp32),
    bits = jax.random.bits(fold_in(key, site), (n,)), i row-major"""
    n = int(np.prod(shape))
    ck = (key, site, n, p)
    if ck not in _MASKS:
        k_site = jax_prng.threefry2x32(key, (0, site))
        h = (n + 1) // 2
        cnt = np.concatenate([np.arange(n, dtype=np.uint32), np.zeros(n % 2, dtype=np.uint32)])
        with np.errstate(over="ignore"):
            y0, y1 = _threefry(k_site, cnt[:h], cnt[h:])
        bits = np.concatenate([y0, y1])[:n]
        u = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
        _MASKS[ck] = (u < np.float32(1.0) - np.float32(p)).astype(np.float64)
    return torch.from_numpy(_MASKS[ck]).reshape(shape) / (1.0 - p)


def test_vectorised_restatement_equals_jax_prng():
    for n in (1, 6, 101):
        k_site = jax_prng.threefry2x32(KEY, (0, 4))
        bits = np.asarray(jax_prng.random_bits(k_site, n), dtype=np.uint32)
        u = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
        exp = (u < np.float32(0.75)).astype(np.float64) / 0.75
        np.testing.assert_array_equal(keep_mask(KEY, 4, (n,), 0.25).numpy(), exp)


# ------------------------------------------------------------------------------------------------ float64 oracle
def oracle_forward(sd, ids, am, pos, key=None, rates=RATES, eps=1e-5):
    """HF GPT-2 blocks in float64 -> final hidden states [B, T, d]; key None: no dropout"""
    import math
    from oracle.gpt2 import gelu_new, layer_norm
    Bq, Tq = ids.shape
    drop = (lambda x, site, p: x * keep_mask(key, site, tuple(x.shape), p)) if key is not None else (lambda x, site, p: x)
    x = drop(sd["wte.weight"][ids] + sd["wpe.weight"][pos], 0, rates["embd_pdrop"])
    hd = D // NH
    mask = torch.tril(torch.ones(Tq, Tq, dtype=torch.bool))[None, None] & am[:, None, None, :].bool()
    for l in range(NL):
        p = f"h.{l}."
        h = layer_norm(x, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"], eps)
        qkv = h @ sd[p + "attn.c_attn.weight"] + sd[p + "attn.c_attn.bias"]
        q, k, v = (t.reshape(Bq, Tq, NH, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
        att = ((q @ k.transpose(-1, -2)) / math.sqrt(hd)).masked_fill(~mask, float("-inf")).softmax(-1)
        att = drop(att, 1 + 3 * l, rates["attn_pdrop"])
        a = (att @ v).transpose(1, 2).reshape(Bq, Tq, D)
        x = x + drop(a @ sd[p + "attn.c_proj.weight"] + sd[p + "attn.c_proj.bias"], 2 + 3 * l, rates["resid_pdrop"])
        h = layer_norm(x, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"], eps)
        m = gelu_new(h @ sd[p + "mlp.c_fc.weight"] + sd[p + "mlp.c_fc.bias"]) @ sd[p + "mlp.c_proj.weight"] + sd[p + "mlp.c_proj.bias"]
        x = x + drop(m, 3 + 3 * l, rates["resid_pdrop"])
    return layer_norm(x, sd["ln_f.weight"], sd["ln_f.bias"], eps)


def _model(seed):
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    cfg = GPT2Config(NL, NH, D, DFF, V, 128)
    sd = init_hf_style_state_dict(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    for k in sd:     # non-trivial biases / LayerNorm parameters, weights above the 0.02 init: no vanishing gradients
        sd[k] = sd[k] * 2 + (0.1 * torch.randn(sd[k].shape, generator=g) if sd[k].dim() == 1 else 0)
    return cfg, sd


def _batch(seed, t=T):
    rng = np.random.RandomState(seed)
    ids = rng.randint(1, PAD, size=(B, t)).astype(np.int32)
    lens = [t, min(50, t - 3), t - 1]
    for b in range(B):
        ids[b, lens[b]:] = PAD
    sta = np.zeros((B, t - 1), dtype=bool)
    for b in range(B):
        for i in range(3, lens[b] - 1):
            sta[b, i] = ((i - 3) // 5) % 2 == 0
    return rng, ids, sta


def _am_pos(ids):
    am = torch.from_numpy((ids != PAD).astype(np.int64))
    return am, (am.cumsum(-1) - 1).clamp(min=0)


def _close(got, exp, rtol, name=""):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    scale = max(float(np.abs(exp).max()), 1e-12)
    err = float(np.abs(got - exp).max()) / scale
    print(f"  {name}: max error {err:.3e} of the largest entry (bound {rtol:.0e})")
    np.testing.assert_allclose(got, exp, rtol=rtol, atol=rtol * scale, err_msg=name)


def _flat_logs(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flat_logs(v, prefix + k + "."))
        else:
            out[prefix + k] = float(v)
    return out


def _dev_inputs(ids, dev):
    am, pos = _am_pos(ids)
    return (torch.from_numpy(ids).to(dev), am.to(torch.uint8).to(dev), pos.to(torch.int32).to(dev))


def _fwd_bwd(dev, sd, ids, w, key, **kw):
    """hidden [B*T, d] and the gradient arena of sum(hidden * w) on the device"""
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32
    m = GPT2F32({k: v.clone() for k, v in sd.items()}, NH, device=dev, **kw)
    hid, cache = m.forward(*_dev_inputs(ids, dev), dropout_key=key)
    grads = m.zero_grads()
    m.backward(cache, w.reshape(B * T, D).to(torch.float32).to(dev).contiguous(), grads)
    return hid.cpu().clone(), {k: v.cpu().clone() for k, v in grads.items()}


@pytest.fixture(scope="module")
def fixed():
    """model, batch, the linear functional's weights (zero on padded positions: no loss reads those rows) and the float64 reference, computed once"""
    cfg, sd = _model(5)
    _, ids, _ = _batch(17)
    am, pos = _am_pos(ids)
    w = torch.randn(B, T, D, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * am[..., None]
    idt = torch.from_numpy(ids).long()
    psd = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    hid = oracle_forward(psd, idt, am, pos, KEY)
    (hid * w).sum().backward()
    with torch.no_grad():
        hid0 = oracle_forward({k: v.double() for k, v in sd.items()}, idt, am, pos, None)
    psd0 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    (oracle_forward(psd0, idt, am, pos, None) * w).sum().backward()
    return dict(sd=sd, ids=ids, w=w, hid=hid.detach(), grads={k: v.grad for k, v in psd.items()}, hid0=hid0, grads0={k: v.grad for k, v in psd0.items()})


# ------------------------------------------------------------------------------------------------ 1. forward / backward against the oracle
@pytest.mark.parametrize("attention", ["flash", "materialized"])
def test_forward_backward_against_float64_oracle(dev, fixed, attention):
    # the test discriminates: the oracle run WITHOUT masks misses both bounds by three orders of magnitude (computed on the CPU: the hidden
    # states by 7.6e3 x the bound, every gradient by 1.1e3 - 4.1e3 x) — except d/d ln_f.bias = sum of the functional's weights, which no mask reaches
    hs = float(fixed["hid"].abs().max())
    assert float((fixed["hid0"] - fixed["hid"]).abs().max()) > 1000 * 1e-4 * hs
    for k, g in fixed["grads"].items():
        if k != "ln_f.bias":
            assert float((fixed["grads0"][k] - g).abs().max()) > 1000 * 3e-4 * float(g.abs().max()), k
    hid, grads = _fwd_bwd(dev, fixed["sd"], fixed["ids"], fixed["w"], KEY, attention=attention, **RATES)
    _close(hid.reshape(B, T, D), fixed["hid"], 1e-4, "hidden")
    for k, g in fixed["grads"].items():
        _close(grads[k], g, 3e-4, k)


# ------------------------------------------------------------------------------------------------ 2. flash versus materialized
def test_flash_equals_materialized_under_dropout(dev, fixed):
    hf, gf = _fwd_bwd(dev, fixed["sd"], fixed["ids"], fixed["w"], KEY, attention="flash", **RATES)
    hm, gm = _fwd_bwd(dev, fixed["sd"], fixed["ids"], fixed["w"], KEY, attention="materialized", **RATES)
    _close(hf, hm, 1e-4, "hidden")
    for k in gm:
        _close(gf[k], gm[k], 3e-4, k)


# ------------------------------------------------------------------------------------------------ 3. + 4. checkpointing, keys
@pytest.mark.parametrize("attention", ["flash", "materialized"])
def test_checkpointing_and_keys(dev, fixed, attention):
    run = lambda key, **kw: _fwd_bwd(dev, fixed["sd"], fixed["ids"], fixed["w"], key, attention=attention, **RATES, **kw)
    h0, g0 = run(KEY)
    h1, g1 = run(KEY, gradient_checkpointing=True)
    h2, g2 = run(KEY)
    h3, g3 = run(KEY2)
    assert torch.equal(h0, h1) and torch.equal(h0, h2)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"gradient checkpointing changed {k}"
        assert torch.equal(g0[k], g2[k]), f"the same key twice gave different {k}"
    assert not torch.equal(h0, h3)
    # (d/d ln_f.bias is the column sum of the functional's weights: no mask reaches it, it is the same under every key)
    assert torch.equal(g0["ln_f.bias"], g3["ln_f.bias"])
    same = [k for k in g0 if k != "ln_f.bias" and torch.equal(g0[k], g3[k])]
    assert not same, f"two keys gave identical gradients for {same}"
    assert jax_prng.as_key(7) == jax_prng.prng_key(7)
    h4, _ = run(7)
    h5, _ = run(jax_prng.prng_key(7))
    assert torch.equal(h4, h5)              # an int seed is prng_key(seed)


# ------------------------------------------------------------------------------------------------ 5. rates at zero
@pytest.mark.parametrize("matmul", ["f32", "bf16"])
def test_zero_rates_and_eval_are_bit_identical_to_no_dropout(dev, fixed, matmul):
    from lmrl_gym_amd.algorithms import bc
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32
    h0, g0 = _fwd_bwd(dev, fixed["sd"], fixed["ids"], fixed["w"], None, matmul=matmul)
    h1, g1 = _fwd_bwd(dev, fixed["sd"], fixed["ids"], fixed["w"], KEY, matmul=matmul)                    # rates 0, key given
    h2, g2 = _fwd_bwd(dev, fixed["sd"], fixed["ids"], fixed["w"], None, matmul=matmul, **RATES)          # rates > 0, no key
    assert torch.equal(h0, h1) and torch.equal(h0, h2)
    for k in g0:
        assert torch.equal(g0[k], g1[k]) and torch.equal(g0[k], g2[k]), k
    # train=False with rates > 0 == rates 0 (a key is given: evaluation must not use it)
    is_action = np.concatenate([np.zeros((B, 1), bool), _batch(17)[2]], axis=1)
    losses = []
    for rates in (RATES, {}):
        m = GPT2F32({k: v.clone() for k, v in fixed["sd"].items()}, NH, device=dev, matmul=matmul, **rates)
        losses.append(bc.GPT2BCTrain(m, PAD, non_action_weight=0.3).step(fixed["ids"], is_action, train=False, prng_key=KEY)[1])
    assert losses[0] == losses[1]


# ------------------------------------------------------------------------------------------------ 6. ILQL step
def _ilql_case():
    cfg, sd = _model(7)
    _, tsd = _model(8)
    rng, ids, sta = _batch(9)
    _, nids, _ = _batch(21, t=24)
    rewards = (rng.randn(B, T - 1) * sta).astype(np.float32)
    dones, next_dones = np.array([1, 0, 0], dtype=np.float32), np.array([0, 1, 0], dtype=np.float32)
    g = torch.Generator().manual_seed(11)
    mk = lambda out: {"dense1.kernel": torch.randn(D, D, generator=g) * 0.05, "dense1.bias": torch.randn(D, generator=g) * 0.1,
                      "dense2.kernel": torch.randn(D, out, generator=g) * 0.05, "dense2.bias": torch.full((out,), -0.4)}
    return dict(sd=sd, tsd=tsd, ids=ids, sta=sta, nids=nids, rewards=rewards, dones=dones, next_dones=next_dones, heads=[mk(V), mk(V), mk(1)],
                kw=dict(gamma=0.99, tau=0.7, cql_weight=0.01))


def _ilql_step(dev, c, matmul, rates, key):
    from lmrl_gym_amd.algorithms import ilql
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, MLPHeadF32
    base = GPT2F32({k: v.clone() for k, v in c["sd"].items()}, NH, device=dev, matmul=matmul, **rates)
    tbase = GPT2F32({k: v.clone() for k, v in c["tsd"].items()}, NH, device=dev, matmul=matmul, **rates)
    heads = [MLPHeadF32({k: v.clone() for k, v in h.items()}, dev, matmul=matmul) for h in c["heads"]]
    tr = ilql.GPT2ILQLTrain(base, *heads, PAD, c["kw"], target_base=tbase, lr=1e-4, polyak_alpha=0.005)
    _, loss, logs = tr.step(c["ids"], c["sta"], c["rewards"], c["dones"], next_token_ids=c["nids"], next_dones=c["next_dones"], prng_key=key)
    return loss, _flat_logs(logs), [{k: v.cpu().clone() for k, v in g.items()} for g in tr.last_grads]


def test_ilql_step_with_dropout_against_float64_oracle(dev):
    """Three model forwards — base, target base, next tokens — under three different keys, in the reference's split order
    (ilql/gpt2/interface.py:132-177): `prng_key, new_key = split(prng_key)` before each call, new_key to the call."""
    from oracle import rl
    c = _ilql_case()
    carry, k_base = jax_prng.split(KEY)
    carry, k_target = jax_prng.split(carry)
    carry, k_next = jax_prng.split(carry)
    assert len({k_base, k_target, k_next}) == 3
    ids, nids = c["ids"], c["nids"]
    am, pos = _am_pos(ids)
    nam, npos = _am_pos(nids)
    idt = torch.from_numpy(ids).long()
    psd = {k: v.double().requires_grad_(True) for k, v in c["sd"].items()}
    req = lambda h: {k: v.double().requires_grad_(True) for k, v in h.items()}
    rq1, rq2, rv = (req(h) for h in c["heads"])
    hid = oracle_forward(psd, idt, am, pos, k_base)
    with torch.no_grad():
        thid = oracle_forward({k: v.double() for k, v in c["tsd"].items()}, idt, am, pos, k_target)
        nhid = oracle_forward({k: v.detach() for k, v in psd.items()}, torch.from_numpy(nids).long(), nam, npos, k_next)
    mh = lambda x, h: rl.mlp_head(x, h["dense1.kernel"], h["dense1.bias"], h["dense2.kernel"], h["dense2.bias"])
    det = lambda h: {k: v.detach() for k, v in h.items()}
    q1o, q2o, vo = mh(hid, rq1), mh(hid, rq2), mh(hid, rv)
    q1, q2, v, v_final, tq1, tq2 = rl.ilql_gather_qv(q1o, q2o, vo, mh(thid, det(rq1)), mh(thid, det(rq2)), idt, am, torch.from_numpy(c["sta"]),
                                                     torch.from_numpy(c["dones"]), next_v_head_out=mh(nhid, det(rv)), next_attention_mask=nam,
                                                     next_dones=torch.from_numpy(c["next_dones"]))
    loss_ref, logs_ref = rl.ilql_loss(q1, q2, v, v_final, tq1, tq2, q1o[:, :-1], q2o[:, :-1], idt[:, 1:], am[:, 1:].double(),
                                      torch.from_numpy(c["sta"]), torch.from_numpy(c["rewards"]).double(), **c["kw"])
    loss_ref.backward()
    loss, logs, (bg, g1, g2, gv) = _ilql_step(dev, c, "f32", RATES, KEY)
    print(f"  loss {loss:.8f} vs float64 {float(loss_ref):.8f}")
    assert abs(loss - float(loss_ref)) <= 1e-4 * abs(float(loss_ref)), (loss, float(loss_ref))
    rf = _flat_logs(logs_ref)
    assert set(rf) == set(logs)
    for k in rf:
        assert abs(logs[k] - rf[k]) <= 1e-4 * max(1.0, abs(rf[k])), (k, logs[k], rf[k])
    for k in psd:
        _close(bg[k], psd[k].grad, 3e-4, k)
    for got, ref in ((g1, rq1), (g2, rq2), (gv, rv)):
        for k in ref:
            _close(got[k], ref[k].grad, 3e-4, k)


# ------------------------------------------------------------------------------------------------ 7. MC and BC steps
def test_mc_step_with_dropout_against_float64_oracle(dev):
    from lmrl_gym_amd.algorithms import mc_returns as mc
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, MLPHeadF32
    from oracle import rl
    c = _ilql_case()
    ids, sta, hq = c["ids"], c["sta"], c["heads"][0]
    am, pos = _am_pos(ids)
    idt = torch.from_numpy(ids).long()
    ret = c["rewards"]
    _, k_base = jax_prng.split(KEY)              # mc_returns/gpt2/interface.py:81-92: one split, new_key to the base model
    psd = {k: v.double().requires_grad_(True) for k, v in c["sd"].items()}
    rq = {k: v.double().requires_grad_(True) for k, v in hq.items()}
    hid = oracle_forward(psd, idt, am, pos, k_base)
    qo = rl.mlp_head(hid, rq["dense1.kernel"], rq["dense1.bias"], rq["dense2.kernel"], rq["dense2.bias"])
    q = qo[:, :-1].gather(2, idt[:, 1:].unsqueeze(-1)).squeeze(2)
    lref, logs_ref = rl.mc_loss(q, qo[:, :-1], idt[:, 1:], am[:, 1:].double(), torch.from_numpy(sta), torch.from_numpy(ret).double(), cql_weight=0.05)
    lref.backward()
    base = GPT2F32({k: v.clone() for k, v in c["sd"].items()}, NH, device=dev, **RATES)
    tr = mc.GPT2MCTrain(base, MLPHeadF32({k: v.clone() for k, v in hq.items()}, dev), PAD, dict(cql_weight=0.05), lr=1e-4)
    _, loss, logs = tr.step(ids, sta, ret, prng_key=KEY)
    assert abs(loss - float(lref)) <= 1e-4 * abs(float(lref)), (loss, float(lref))
    rf, gf = _flat_logs(logs_ref), _flat_logs(logs)
    for k in rf:
        assert abs(gf[k] - rf[k]) <= 1e-4 * max(1.0, abs(rf[k])), (k, gf[k], rf[k])
    for k in psd:
        _close(tr.last_grads[0][k].cpu(), psd[k].grad, 3e-4, k)
    for k in rq:
        _close(tr.last_grads[1][k].cpu(), rq[k].grad, 3e-4, k)


def test_bc_step_with_dropout_against_float64_oracle(dev):
    from lmrl_gym_amd.algorithms import bc
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32
    from oracle import rl
    c = _ilql_case()
    ids = c["ids"]
    am, pos = _am_pos(ids)
    is_action = np.concatenate([np.zeros((B, 1), bool), c["sta"]], axis=1)
    psd = {k: v.double().requires_grad_(True) for k, v in c["sd"].items()}
    hid = oracle_forward(psd, torch.from_numpy(ids).long(), am, pos, KEY)       # bc/interface.py:39, :121-131: the step's rng IS the dropout rng
    lref = rl.bc_loss(hid @ psd["wte.weight"].t(), torch.from_numpy(ids), am, torch.from_numpy(is_action), non_action_weight=0.3)
    lref.backward()
    m = GPT2F32({k: v.clone() for k, v in c["sd"].items()}, NH, device=dev, **RATES)
    trb = bc.GPT2BCTrain(m, PAD, non_action_weight=0.3, lr=1e-4)
    _, loss, _ = trb.step(ids, is_action, prng_key=KEY)
    assert abs(loss - float(lref)) <= 1e-4 * abs(float(lref)), (loss, float(lref))
    for k in psd:
        _close(trb.last_grads[k].cpu(), psd[k].grad, 3e-4, k)


# ------------------------------------------------------------------------------------------------ 8. bf16-matmul mode
def _grad_figures(g0, g1):
    out = {}
    for gi, (a_, b_) in enumerate(zip(g0, g1)):
        for k in a_:
            a, b = a_[k].reshape(-1).double(), b_[k].reshape(-1).double()
            na = float(a.norm())
            if na < 1e-12:
                assert float(b.norm()) < 1e-9, k
                continue
            out[(gi, k)] = (float((a - b).norm()) / na, float((a * b).sum()) / (na * float(b.norm())))
    return out


def test_bf16_matmul_ilql_step_with_dropout(dev):
    """The ILQL step in bf16-matmul mode against our fp32 step, same key: the masks are identical by construction, so the difference is the
    mode's operand rounding alone.  Bounds of tests/test_gpu_train_bf16.py: loss 2e-2, gradient relative L2 <= 0.10, cosine >= 0.995.  A tensor
    beyond them is compared with its figure for the same two steps WITHOUT dropout, measured here, and may reach 1.5 x that (relative L2, and
    1 - cosine); the test prints the worst tensor's figures of both pairs."""
    c = _ilql_case()
    l0, _, g0 = _ilql_step(dev, c, "f32", RATES, KEY)
    l1, _, g1 = _ilql_step(dev, c, "bf16", RATES, KEY)
    n0, _, h0 = _ilql_step(dev, c, "f32", {}, None)
    n1, _, h1 = _ilql_step(dev, c, "bf16", {}, None)
    print(f"  loss fp32 {l0:.6f} bf16 {l1:.6f} (no dropout: {n0:.6f} / {n1:.6f})")
    assert abs(l1 - l0) <= 2e-2 * max(abs(l0), 0.05), (l0, l1)
    fd, fn = _grad_figures(g0, g1), _grad_figures(h0, h1)
    worst_d, worst_n = max(fd.items(), key=lambda kv: kv[1][0]), max(fn.items(), key=lambda kv: kv[1][0])
    print(f"  worst gradient tensor with dropout {worst_d[0]}: relative L2 {worst_d[1][0]:.4f}, cosine {worst_d[1][1]:.5f}; "
          f"without {worst_n[0]}: {worst_n[1][0]:.4f}, {worst_n[1][1]:.5f}")
    for k, (rel, cos) in fd.items():
        if rel <= 0.10 and cos >= 0.995:
            continue
        rel_n, cos_n = fn[k]
        assert rel <= 1.5 * rel_n and (1 - cos) <= 1.5 * (1 - cos_n), (k, rel, cos, rel_n, cos_n)


# ------------------------------------------------------------------------------------------------ 9. missing key
def test_train_with_rates_and_no_key_raises(dev):
    from lmrl_gym_amd.algorithms import bc, mc_returns as mc
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, MLPHeadF32
    c = _ilql_case()
    is_action = np.concatenate([np.zeros((B, 1), bool), c["sta"]], axis=1)
    m = GPT2F32({k: v.clone() for k, v in c["sd"].items()}, NH, device=dev, **RATES)
    with pytest.raises(ValueError):
        bc.GPT2BCTrain(m, PAD).step(c["ids"], is_action)
    with pytest.raises(ValueError):
        mc.GPT2MCTrain(m, MLPHeadF32({k: v.clone() for k, v in c["heads"][0].items()}, dev), PAD, dict(cql_weight=0.05)).step(c["ids"], c["sta"], c["rewards"])
    with pytest.raises(ValueError):
        _ilql_step(dev, c, "f32", RATES, None)
    with pytest.raises(ValueError):
        GPT2F32({k: v.clone() for k, v in c["sd"].items()}, NH, device=dev, attn_pdrop=1.0)
