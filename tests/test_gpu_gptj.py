"""GPU tier of the GPT-J fp32 engine (`lmrl_gym_amd.gptj_f32_engine`, csrc/attn_rope_f32.hip), all through the C ABI.

Oracles: float64 numpy restatements for the two kernels, and for the engine the installed `transformers` PyTorch `GPTJForCausalLM` run on the CPU in
float64 (`model.double()`) on LEFT-padded batches with an attention mask and mask-derived position ids (`cumsum(mask) - 1`, what the reference's
`initialize_attn_mask_pos_ids` hands its models) — so the engine's per-env cache positions are checked to mean what the reference's positions mean.

Attention tolerance (test 2).  T = 8 is the key-tile size of `lmrl_attn_cached_hd_f32` (`lmrl_attn_hd_key_tile()`).  The bound is derived from the
EXISTING kernel's own error, measured in the test on the head_dim = 64 inputs of the same schedule and batch: e64 = max |lmrl_attn_cached_f32 -
float64|; the new entry is allowed 2 e64 at head_dim 64 (a different association order), and 2 e64 head_dim / 64 at 128 and 256 (dot products that
much longer).  Measured on an MI355X (q, k, v ~ N(0, 1); max abs error, bound in brackets; also in DESIGN.md §6h):
    B = 3:   e64 = 3.31e-7; new entry 3.31e-7 at 64 (6.62e-7), 4.50e-7 at 128 (1.32e-6), 3.54e-7 at 256 (2.65e-6)
    B = 33:  e64 = 4.30e-7; new entry 4.30e-7 at 64 (8.59e-7), 4.43e-7 at 128 (1.72e-6), 5.90e-7 at 256 (3.44e-6)

The HF oracle's eager `_attn` casts q and k to float32 for the scores whatever the model's dtype, so "HF float64" carries fp32 rounding in its scores:
measured on the CPU it lies within 5e-6 (relative to the largest entry) of an all-float64 restatement of the block — inside the 2e-5 bound of test 3,
far below the 2e-4 tie thresholds of tests 4 and 5.
"""
import ctypes

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T_KEY = 8            # key positions per tile of the head-dim attention kernel (csrc/attn_rope_f32.hip: kKeyTile)
SHAPES = {           # the engine shapes of the issue: (a) head dim 256, (b) head dim 64, (c) head dim 128 with the whole head rotated
    "a": dict(n_layer=2, n_head=2, d_model=512, rotary_dim=64, vocab=96, n_pos=64),
    "b": dict(n_layer=2, n_head=4, d_model=256, rotary_dim=16, vocab=96, n_pos=64),
    "c": dict(n_layer=2, n_head=2, d_model=256, rotary_dim=None, vocab=96, n_pos=64),
}
GREEDY_SEED = 3      # weight seed of test 4, chosen on the CPU: the HF float64 model's own greedy run has no top-2 gap below 2e-4 (see the test)


@pytest.fixture(scope="module")
def dev():
    from lmrl_gym_amd import _lib
    return _lib.require_gpu()


def _cfg(shape):
    from lmrl_gym_amd.gptj_f32_engine import GPTJConfig
    return GPTJConfig(**SHAPES[shape])


def _weights(cfg, seed, scale=3.0):
    """HF-style init, widened (x scale on matrices) and with non-trivial LayerNorm parameters and biases, so that no term of the block is inert."""
    from lmrl_gym_amd.gptj_f32_engine import init_hf_style_gptj_state_dict
    sd = init_hf_style_gptj_state_dict(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    return {k: v * scale + 0.1 * torch.randn(v.shape, generator=g) if v.dim() == 1 else v * scale for k, v in sd.items()}


def _hf_model(cfg, sd):
    from transformers import GPTJConfig as HFConfig, GPTJForCausalLM
    hf = GPTJForCausalLM(HFConfig(**cfg.to_hf(), attn_implementation="eager", attn_pdrop=0.0, embd_pdrop=0.0, resid_pdrop=0.0))
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(("attn.bias", "attn.masked_bias", "embed_positions")) for k in missing), (missing, unexpected)
    return hf.double().eval()


def _hf_forward(hf, seqs):
    """Left-padded batch -> per env (logits [n, V], ln_f hidden [n, d]) float64 numpy, aligned with the env's own n tokens."""
    Tm = max(len(s) for s in seqs)
    ids = torch.zeros(len(seqs), Tm, dtype=torch.long)
    mask = torch.zeros(len(seqs), Tm, dtype=torch.long)
    for b, s in enumerate(seqs):
        ids[b, Tm - len(s):] = torch.tensor(s, dtype=torch.long)
        mask[b, Tm - len(s):] = 1
    pos = torch.clamp(torch.cumsum(mask, dim=1) - 1, min=0)
    with torch.no_grad():
        out = hf(input_ids=ids, attention_mask=mask, position_ids=pos, output_hidden_states=True, use_cache=False)
    lg, hid = out.logits.numpy(), out.hidden_states[-1].numpy()
    return [(lg[b, Tm - len(s):], hid[b, Tm - len(s):]) for b, s in enumerate(seqs)]


def _dt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------------ 1. rotary kernel
@pytest.mark.parametrize("head_dim,rotary_dim", [(64, 16), (64, 64), (256, 16), (256, 64), (256, 256)])
def test_rope_kernel_vs_float64(dev, head_dim, rotary_dim):
    """In-place rotation of q and k against a float64 restatement on the same fp32 inputs and the same fp32 table.  Per-element bound
    4 * 2^-24 * (|x[2i]| + |x[2i+1]|): two rounded products and one rounded add, |sin|, |cos| <= 1.  v, the dims past rotary_dim and the rows with
    pos = -1 come back bit-identical; pos = n_pos is an error status of the checking entry (and a pass-through of the capturable one)."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gptj_f32_engine import rotary_sincos_table
    L = _lib.lib()
    rows, H, n_pos, half = 37, 2, 64, rotary_dim // 2
    d = H * head_dim
    rng = np.random.RandomState(head_dim + rotary_dim)
    x = rng.standard_normal((rows, 3 * d)).astype(np.float32)
    pos = rng.randint(0, n_pos, size=rows).astype(np.int32)
    pos[:6] = [0, 32, 47, 63, 1, 33]                     # position 0 is the identity: every case rotates at positions >= 32 too
    dead = [9, 17, 36]
    pos[dead] = -1
    assert (pos >= 32).sum() >= 4
    table = rotary_sincos_table(n_pos, rotary_dim)
    tab_d, pos_d = table.to(dev), _dt(pos, dev)
    outs = []
    for entry in (L.lmrl_rope_gptj_f32, L.lmrl_rope_gptj_f32_async):
        buf = _dt(x, dev)
        _lib.check(entry(_lib.ptr(buf), _lib.ptr(pos_d), _lib.ptr(tab_d), rows, H, head_dim, rotary_dim, n_pos, _lib.stream_ptr()), "rope")
        torch.cuda.synchronize()
        outs.append(buf.cpu().numpy())
    got = outs[0]
    assert np.array_equal(got.view(np.uint32), outs[1].view(np.uint32))            # one kernel behind both entries
    tab = table.numpy().astype(np.float64)
    ref = x.astype(np.float64).copy().reshape(rows, 3, H, head_dim)
    bound = np.zeros_like(ref)
    xr = x.astype(np.float64).reshape(rows, 3, H, head_dim)
    for r in range(rows):
        if pos[r] < 0:
            continue
        sn, cs = tab[pos[r], :half], tab[pos[r], half:]
        for w in (0, 1):                                                           # q and k; v (2) is not rotated
            x0, x1 = xr[r, w, :, 0:rotary_dim:2], xr[r, w, :, 1:rotary_dim:2]
            ref[r, w, :, 0:rotary_dim:2] = x0 * cs - x1 * sn
            ref[r, w, :, 1:rotary_dim:2] = x1 * cs + x0 * sn
            b = 4.0 * 2.0 ** -24 * (np.abs(x0) + np.abs(x1))
            bound[r, w, :, 0:rotary_dim:2] = b
            bound[r, w, :, 1:rotary_dim:2] = b
    g4 = got.reshape(rows, 3, H, head_dim)
    err = np.abs(g4.astype(np.float64) - ref)
    print("rope head_dim %d rotary_dim %d: max err %.3e, max err / bound %.3f" % (head_dim, rotary_dim, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    x4 = x.reshape(rows, 3, H, head_dim)
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert same(g4[:, 2], x4[:, 2])                                                # v
    assert same(g4[:, :, :, rotary_dim:], x4[:, :, :, rotary_dim:])                # pass-through dims
    assert same(g4[dead], x4[dead])                                                # dead slots
    live = [r for r in range(rows) if pos[r] > 0]
    assert not same(g4[live][:, :2, :, :rotary_dim], x4[live][:, :2, :, :rotary_dim])
    # pos = n_pos: an error status and no launch from the checking entry; the capturable entry leaves such a row alone (never reads the table)
    bad = pos.copy()
    bad[5] = n_pos
    bad_d, buf = _dt(bad, dev), _dt(x, dev)
    rc = L.lmrl_rope_gptj_f32(_lib.ptr(buf), _lib.ptr(bad_d), _lib.ptr(tab_d), rows, H, head_dim, rotary_dim, n_pos, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"position" in L.lmrl_last_error() and same(buf.cpu().numpy(), x)
    _lib.check(L.lmrl_rope_gptj_f32_async(_lib.ptr(buf), _lib.ptr(bad_d), _lib.ptr(tab_d), rows, H, head_dim, rotary_dim, n_pos, _lib.stream_ptr()), "rope")
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert same(after[5], x[5]) and same(np.delete(after, 5, axis=0), np.delete(got, 5, axis=0))
    for hd, rd in ((head_dim, rotary_dim + 1), (head_dim, head_dim + 2)):          # odd / oversized rotary_dim
        assert L.lmrl_rope_gptj_f32(_lib.ptr(buf), _lib.ptr(pos_d), _lib.ptr(tab_d), rows, H, hd, rd, n_pos, _lib.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------------------------ 2. attention kernel
def _attn_schedule(B):
    """(C, cnt[B]) per call: two ragged 8-token chunks (counts 0..8, a 0 and an 8 among them), then 12 single-token decodes (two of them ragged)."""
    base1, base2 = [7, 8, 0, 3, 8, 1, 5], [1, 8, 0, 5, 0, 8, 2]
    cyc = lambda base: np.array([base[b % len(base)] for b in range(B)], dtype=np.int32)
    calls = [(8, cyc(base1)), (8, cyc(base2))]
    for s in range(12):
        c = np.ones(B, dtype=np.int32)
        if s in (3, 8):
            c[1::3] = 0
        calls.append((1, c))
    return calls


def _run_attention(dev, entry, head_dim, B, seed):
    """Drive one attention entry through `_attn_schedule` on random fp32 q / k / v -> (max |out - float64|, cache lengths seen at call time).
    Also checks, bit for bit, that the cache rows written are the appended k and v, and that nothing else was written."""
    from lmrl_gym_amd import _lib
    H, tmax = 2, 40
    d = H * head_dim
    rng = np.random.RandomState(seed)
    kc = torch.zeros(B, tmax, d, dtype=torch.float32, device=dev)
    vc = torch.zeros(B, tmax, d, dtype=torch.float32, device=dev)
    lens = np.zeros(B, dtype=np.int32)
    Ks = [np.zeros((0, d), np.float32) for _ in range(B)]
    Vs = [np.zeros((0, d), np.float32) for _ in range(B)]
    worst, seen = 0.0, set()
    for C, cnt in _attn_schedule(B):
        qkv = rng.standard_normal((B * C, 3 * d)).astype(np.float32)
        out_d = torch.full((B * C, d), 777.0, dtype=torch.float32, device=dev)
        seen.update(int(x) for x in lens)
        qkv_d, len_d, cnt_d = _dt(qkv, dev), _dt(lens, dev), _dt(cnt, dev)
        _lib.check(entry(_lib.ptr(qkv_d), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(len_d), _lib.ptr(cnt_d), _lib.ptr(out_d), B, C, H, tmax), "attention")
        torch.cuda.synchronize()
        out = out_d.cpu().numpy()
        for b in range(B):
            rows = qkv[b * C: b * C + cnt[b]]
            Ks[b] = np.concatenate([Ks[b], rows[:, d:2 * d]])
            Vs[b] = np.concatenate([Vs[b], rows[:, 2 * d:]])
            for j in range(C):
                if j >= cnt[b]:
                    assert (out[b * C + j] == 777.0).all()                         # padding slots untouched
                    continue
                n = lens[b] + j + 1
                for h in range(H):
                    sl = slice(h * head_dim, (h + 1) * head_dim)
                    q = rows[j, sl].astype(np.float64)
                    s = Ks[b][:n, sl].astype(np.float64) @ q / np.sqrt(float(head_dim))
                    p = np.exp(s - s.max())
                    ref = (p / p.sum()) @ Vs[b][:n, sl].astype(np.float64)
                    worst = max(worst, float(np.abs(out[b * C + j, sl] - ref).max()))
            lens[b] += cnt[b]
    kh, vh = kc.cpu().numpy(), vc.cpu().numpy()
    for b in range(B):
        n = lens[b]
        assert np.array_equal(kh[b, :n].view(np.uint32), Ks[b].view(np.uint32)) and np.array_equal(vh[b, :n].view(np.uint32), Vs[b].view(np.uint32))
        assert not kh[b, n:].any() and not vh[b, n:].any()
    return worst, seen


_E64 = {}


def _existing_kernel_error(dev, B):
    """e64: the error of the existing head-dim-64 entry against the same float64 formula on the head_dim = 64 inputs (once per batch size)."""
    from lmrl_gym_amd import _lib
    if B not in _E64:
        L = _lib.lib()
        old = lambda qkv, k, v, ln, cnt, out, b, c, h, tmax: L.lmrl_attn_cached_f32(qkv, k, v, ln, cnt, out, b, c, h, tmax, _lib.stream_ptr())
        _E64[B] = _run_attention(dev, old, 64, B, seed=640 + B)[0]
    return _E64[B]


@pytest.mark.parametrize("B", [3, 33])
@pytest.mark.parametrize("head_dim", [64, 128, 256])
def test_attention_kernel_vs_float64(dev, head_dim, B):
    """Ragged prefill (C = 8, counts 0..8) then decodes (C = 1) against float64 causal attention on the same fp32 inputs; the cache lengths met
    straddle the kernel's key tile T = 8 (T - 1, T, T + 1, 2 T + 1); tolerance from the existing kernel's measured error (module docstring)."""
    from lmrl_gym_amd import _lib
    L = _lib.lib()
    assert L.lmrl_attn_hd_key_tile() == T_KEY
    e64 = _existing_kernel_error(dev, B)
    new = lambda qkv, k, v, ln, cnt, out, b, c, h, tmax: L.lmrl_attn_cached_hd_f32(qkv, k, v, ln, cnt, out, b, c, h, head_dim, tmax, _lib.stream_ptr())
    err, seen = _run_attention(dev, new, head_dim, B, seed=(640 + B) if head_dim == 64 else head_dim + B)
    bound = 2.0 * e64 * head_dim / 64
    print("attention head_dim %d B %d: existing kernel e64 = %.3e, new entry err = %.3e, bound = %.3e" % (head_dim, B, e64, err, bound))
    assert {T_KEY - 1, T_KEY, T_KEY + 1, 2 * T_KEY + 1} <= seen, sorted(seen)
    assert 0.0 < e64 < 1e-5                                                        # the yardstick itself is at fp32 rounding level
    assert err <= bound, (err, bound)
    if head_dim == 64 and B == 3:
        a = torch.zeros(8, dtype=torch.float32, device=dev)
        assert L.lmrl_attn_cached_hd_f32(_lib.ptr(a), _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), 1, 1, 1, 96, 4, _lib.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------------------------ 3. engine vs HF float64
@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_engine_hidden_states_and_logits_vs_hf_float64(dev, shape):
    """Two ragged 8-token prefill chunks, then 24 single-token decodes (positions reach 39): `all_hidden`, `last_hidden` and the logits of every
    forward against HF float64 on the left-padded batch, at the project's fp32 bound (2e-5 of the largest entry, tests/test_gpu_f32_engine.py)."""
    from lmrl_gym_amd.gptj_f32_engine import GPTJEngineF32
    cfg = _cfg(shape)
    sd = _weights(cfg, seed=11)
    eng = GPTJEngineF32(cfg, sd, dev)
    B, tol = 3, 2e-5
    ses = eng.session(B, 64)
    ses.reset()
    rng = np.random.RandomState(5)
    seqs = [[] for _ in range(B)]
    record = []                                                                    # (cnts, lens before, all_hidden, last_hidden, logits)
    for C, cnts in [(8, [8, 5, 3]), (8, [8, 0, 6])] + [(1, [1, 1, 1])] * 24:
        toks = np.zeros((B, C), dtype=np.int32)
        before = [len(s) for s in seqs]
        for b in range(B):
            new = rng.randint(0, cfg.vocab, size=cnts[b])
            toks[b, : cnts[b]] = new
            seqs[b] += new.tolist()
        allh = torch.zeros(B * C, cfg.d_model, dtype=torch.float32, device=dev)
        ses.forward(_dt(toks.reshape(-1), dev), _dt(np.asarray(cnts, dtype=np.int32), dev), C, all_hidden=allh)
        lg = ses.lm_logits()
        torch.cuda.synchronize()
        assert ses.len.cpu().numpy().tolist() == [len(s) for s in seqs]
        record.append((C, cnts, before, allh.cpu().double().numpy(), ses.last_hidden.cpu().double().numpy(), lg.cpu().double().numpy()))
    assert max(len(s) for s in seqs) - 1 >= 32
    ref = _hf_forward(_hf_model(cfg, sd), seqs)
    worst_h = worst_l = 0.0
    for C, cnts, before, allh, lasth, lg in record:
        assert not lg[:, cfg.vocab:].any()                                         # padded vocabulary rows are zero
        for b in range(B):
            if cnts[b] == 0:
                continue
            ref_lg, ref_h = ref[b]
            for j in range(cnts[b]):
                r = ref_h[before[b] + j]
                e = np.abs(allh[b * C + j] - r).max() / max(1.0, np.abs(r).max())
                worst_h = max(worst_h, e)
                assert e <= tol, ("all_hidden", shape, C, b, j, e)
            last = before[b] + cnts[b] - 1
            e = np.abs(lasth[b] - ref_h[last]).max() / max(1.0, np.abs(ref_h[last]).max())
            worst_h = max(worst_h, e)
            assert e <= tol, ("last_hidden", shape, C, b, e)
            e = np.abs(lg[b, : cfg.vocab] - ref_lg[last]).max() / max(1.0, np.abs(ref_lg[last]).max())
            worst_l = max(worst_l, e)
            assert e <= tol, ("logits", shape, C, b, e)
    print("engine shape %s: worst relative error hidden %.3e, logits %.3e (bound %.0e)" % (shape, worst_h, worst_l, tol))


# ------------------------------------------------------------------------------------------------------------------ 4. greedy generation
def _hf_greedy(hf, prompts, n_new):
    """HF float64 greedy continuation, one full forward per token -> (tokens [B][n_new], top-2 logit gaps [B][n_new])."""
    seqs = [list(p) for p in prompts]
    toks, gaps = np.zeros((len(seqs), n_new), dtype=np.int64), np.zeros((len(seqs), n_new))
    for k in range(n_new):
        for b, (lg, _) in enumerate(_hf_forward(hf, seqs)):
            top = np.sort(lg[-1])[-2:]
            toks[b, k], gaps[b, k] = int(lg[-1].argmax()), top[1] - top[0]
            seqs[b].append(int(toks[b, k]))
    return toks, gaps


def _greedy_prompts(vocab, B=8):
    rng = np.random.RandomState(21)
    return [rng.randint(0, vocab, size=n).tolist() for n in [8, 3, 5, 8, 1, 7, 4, 6][:B]]


def test_greedy_generation_equals_hf_float64(dev):
    """24 greedy tokens, shape (a), B = 8: equal to HF float64 greedy wherever the oracle's top-2 logit gap exceeds 2e-4 (the tie threshold of the
    fp32 rollout test).  At most 0.5 % of the positions may be near-ties: with 192 positions, none — GREEDY_SEED was picked on the CPU so that the HF
    model alone has no gap below 2e-4 (asserted here on the oracle's own numbers)."""
    from lmrl_gym_amd.gpt2 import SampleParams
    from lmrl_gym_amd.gptj_f32_engine import GPTJEngineF32
    cfg, B, N = _cfg("a"), 8, 24
    sd = _weights(cfg, seed=GREEDY_SEED)
    prompts = _greedy_prompts(cfg.vocab, B)
    ref_tok, gaps = _hf_greedy(_hf_model(cfg, sd), prompts, N)
    near = gaps <= 2e-4
    assert near.sum() <= 0.005 * near.size, (int(near.sum()), float(gaps.min()))
    eng = GPTJEngineF32(cfg, sd, dev)
    ses = eng.session(B, 48)
    ses.reset()
    toks = np.zeros((B, 8), dtype=np.int32)
    for b, p in enumerate(prompts):
        toks[b, : len(p)] = p
    ses.forward(_dt(toks.reshape(-1), dev), _dt(np.array([len(p) for p in prompts], dtype=np.int32), dev), 8)
    one = torch.ones(B, dtype=torch.int32, device=dev)
    got = np.zeros((B, N), dtype=np.int64)
    for k in range(N):
        tok, _ = ses.sample(SampleParams(0.0, 0, 1, k, 0.0, 0.0, 0, None, 0.0), want_logprob=False)
        got[:, k] = tok.cpu().numpy()
        ses.forward(tok.clone(), one, 1)
    for b in range(B):
        for k in range(N):
            if near[b, k]:
                break                                                              # past a near-tie the two runs may follow different prefixes
            assert got[b, k] == ref_tok[b, k], (b, k, float(gaps[b, k]))
    assert len({tuple(r) for r in got.tolist()}) > 1                               # not one constant continuation


# ------------------------------------------------------------------------------------------------------------------ 5. sampling
def test_sampled_tokens_equal_the_materialised_sampler_on_hf_float64_logits(dev):
    """Fixed seed, temperature 0.7, top_k = 5, top_p = 0.9, shape (a), B = 16, 24 draws per env: the session's tokens equal those of the existing
    materialised sampler (`lmrl_sample_logits_steer`, same parameters) run on the HF float64 logits of the same prefixes rounded to fp32.  Draws
    whose top-2 perturbed scores (float64 warpers + the sampler's Gumbel noise, both from the oracle) lie within 2e-4 are skipped; < 0.5 % are."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gpt2 import SampleParams
    from lmrl_gym_amd.gptj_f32_engine import GPTJEngineF32
    from oracle import gpt2 as O, warpers as OW
    cfg, B, N, SEED, TEMP, TOPK, TOPP = _cfg("a"), 16, 24, 20240, 0.7, 5, 0.9
    sd = _weights(cfg, seed=7)
    eng = GPTJEngineF32(cfg, sd, dev)
    L = _lib.lib()
    ses = eng.session(B, 48)
    ses.reset()
    rng = np.random.RandomState(9)
    prompts = [rng.randint(0, cfg.vocab, size=1 + (b * 3) % 8).tolist() for b in range(B)]
    toks = np.zeros((B, 8), dtype=np.int32)
    for b, p in enumerate(prompts):
        toks[b, : len(p)] = p
    ses.forward(_dt(toks.reshape(-1), dev), _dt(np.array([len(p) for p in prompts], dtype=np.int32), dev), 8)
    one = torch.ones(B, dtype=torch.int32, device=dev)
    params = lambda k: SampleParams(TEMP, TOPK, SEED, k, 0.0, 0.0, 0, None, TOPP)
    got = np.zeros((B, N), dtype=np.int64)
    for k in range(N):
        tok, _ = ses.sample(params(k), want_logprob=False)
        got[:, k] = tok.cpu().numpy()
        ses.forward(tok.clone(), one, 1)
    seqs = [p + got[b].tolist() for b, p in enumerate(prompts)]
    ref = _hf_forward(_hf_model(cfg, sd), seqs)
    tok_d = torch.zeros(B, dtype=torch.int32, device=dev)
    checked = skipped = 0
    for k in range(N):
        z64 = np.stack([ref[b][0][len(prompts[b]) + k - 1] for b in range(B)])      # logits that produced draw k
        lg = torch.zeros(B, cfg.vocab_padded, dtype=torch.float32)
        lg[:, : cfg.vocab] = torch.from_numpy(z64).float()
        lg_d = lg.to(dev)
        p = params(k)
        _lib.check(L.lmrl_sample_logits_steer(_lib.ptr(lg_d), cfg.vocab_padded, B, cfg.vocab, ctypes.byref(p), None, None, _lib.ptr(tok_d), None,
                                              _lib.stream_ptr()), "lmrl_sample_logits_steer")
        want = tok_d.cpu().numpy()
        zs, keep = OW.warp(z64, TEMP, TOPK, TOPP)
        score = np.where(keep, zs + O.gumbel_noise(B, cfg.vocab, SEED, k).astype(np.float64), -np.inf)
        top2 = np.sort(score, axis=1)[:, -2:]
        for b in range(B):
            if top2[b, 1] - top2[b, 0] < 2e-4:
                skipped += 1
                continue
            checked += 1
            assert int(score[b].argmax()) == int(want[b]) == int(got[b, k]), (b, k, int(score[b].argmax()), int(want[b]), int(got[b, k]))
    print("sampling: %d draws checked, %d near-ties skipped" % (checked, skipped))
    assert checked + skipped == B * N and skipped < 0.005 * (checked + skipped), (checked, skipped)
    assert len(np.unique(got)) > 8                                                 # real sampling, not one token


# ------------------------------------------------------------------------------------------------------------------ 6. hipGraph
def test_graph_replay_of_decode_steps_is_bit_identical_to_eager(dev):
    """8 decode steps (sample + forward) eagerly, then the same steps captured in one `torch.cuda.graph` and replayed from the same cache state:
    bit-identical tokens and `last_hidden`.  One stream, no parallel branches; `forward` neither synchronises nor allocates after its first call."""
    from lmrl_gym_amd.gpt2 import SampleParams
    from lmrl_gym_amd.gptj_f32_engine import GPTJEngineF32
    cfg, B, N = _cfg("b"), 5, 8
    eng = GPTJEngineF32(cfg, _weights(cfg, seed=2), dev)
    ses = eng.session(B, 32)
    ses.reset()
    rng = np.random.RandomState(1)
    cnt0 = np.array([8, 2, 5, 8, 1], dtype=np.int32)
    ses.forward(_dt(rng.randint(0, cfg.vocab, size=B * 8).astype(np.int32), dev), _dt(cnt0, dev), 8)
    one = torch.ones(B, dtype=torch.int32, device=dev)
    toks, hids = torch.zeros(N, B, dtype=torch.int32, device=dev), torch.zeros(N, B, cfg.d_model, dtype=torch.float32, device=dev)

    def steps():
        for k in range(N):
            tok, _ = ses.sample(SampleParams(1.0, 0, 99, k, 0.0, 0.0, 0, None, 0.0), want_logprob=False)
            toks[k].copy_(tok)
            ses.forward(tok, one, 1)
            hids[k].copy_(ses.last_hidden)

    state = lambda: [t.clone() for t in (ses.kv, ses.len, ses._last_x, ses.last_hidden)]

    def restore(snap):
        for t, s in zip((ses.kv, ses.len, ses._last_x, ses.last_hidden), snap):
            t.copy_(s)
        ses._len_bound = int(cnt0.max())
    snap = state()
    steps()                                                                        # eager (also the warm-up: every workspace exists after it)
    torch.cuda.synchronize()
    eager = (toks.clone(), hids.clone())
    restore(snap)
    toks.zero_(); hids.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps()
    restore(snap)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(toks, eager[0]) and torch.equal(hids, eager[1])
    assert ses.len.cpu().numpy().tolist() == (cnt0 + N).tolist() and len(torch.unique(toks)) > 4


# ------------------------------------------------------------------------------------------------------------------ 7. text policies
class _CharTok:
    """One id per ASCII character (0..127): a toy tokenizer for Wordle text; pad = 0, eos = newline."""
    pad_token_id, eos_token_id = 0, 10

    def encode(self, s):
        return [ord(c) if ord(c) < 128 else 63 for c in s]

    def decode(self, ids, **kw):
        return "".join(chr(int(i)) for i in ids if int(i) != 0)


def test_text_policy_end_to_end_with_and_without_kv_reuse(dev):
    """`GPTJPPOPolicy` + `interact_environment` on the Wordle env (400-word vocabulary, character tokenizer), greedy: KV reuse across `act()` calls
    and a fresh session per call give identical `InteractionTransition` lists."""
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.envs import wordle as W
    from lmrl_gym_amd.gptj_f32_engine import GPTJConfig, GPTJEngineF32
    from lmrl_gym_amd.policies import GPTJPPOPolicy
    cfg = GPTJConfig(n_layer=2, n_head=4, d_model=256, rotary_dim=16, vocab=128, n_pos=256)
    sd = _weights(cfg, seed=4)
    letters = [ord(c) for c in "abcdefghijklmnopqrstuvwxyz \n"]
    sd["lm_head.bias"][letters] += 6.0                                             # actions made of Wordle's alphabet (a BC-initialised policy's role)
    eng = GPTJEngineF32(cfg, sd, dev)
    tok = _CharTok()

    class FreshSessions(GPTJPPOPolicy):
        def act(self, text_history, done=None):
            self._gen = None                                                       # a new generator (new KV sessions) for every call
            return super().act(text_history, done)

    kw = dict(max_input_length=160, max_new_tokens=10, do_sample=False, eos_token_id=tok.eos_token_id, out_str_process=lambda x: x.removesuffix("\n") + "\n")
    vocab = W.Vocabulary.builtin("wordle_official_400.txt")
    runs = []
    for policy in (GPTJPPOPolicy(eng, tok, reuse_kv=True, **kw), FreshSessions(eng, tok, reuse_kv=False, **kw)):
        env = W.ReformatWordleEnvironment(vocab, require_words_in_vocab=True, bad_word_reward=-10.0)
        runs.append(E.interact_environment(env, policy, env_seed=[3, 4, 5, 6], bsize=4))
        if policy.reuse_kv:
            reused = policy._gen.prefilled_tokens
    a, b = runs
    assert len(a) == 4 and all(len(ep) >= 2 and ep[-1].done for ep in a)
    assert a == b
    texts = {tr.post_action_history[-1].text for ep in a for tr in ep}
    assert all(t.endswith("\n") for t in texts) and len(texts) > 1
    assert reused < sum(len(tok.encode(E.text_history_to_str(tr.pre_action_history))) for ep in a for tr in ep)      # reuse forwarded less than the full prompts
