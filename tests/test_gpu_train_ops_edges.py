"""GPU tier: the fp32 train ops (csrc/train_ops.hip) at the edges of their kernel paths, each against a plain float64 restatement on the CPU.

`test_train_ops_vs_autograd` (tests/test_gpu_train.py) runs every op once at one toy shape; here every op runs where its code takes another
path: segment boundaries off the 16-byte grid in the arena AdamW sweep, every LayerNorm width with a kernel of its own, rows that start at
each 16-byte phase in the log-softmax kernel, more than one 64-lane sweep in the softmax, slabs of several rows in the column sums, the
grid-stride loop of the elementwise kernels, the scalar paths of gather / scatter and the wider embedding-gradient kernels.

The unmarked tests at the top need no GPU: they check the references themselves (the AdamW restatement against torch.optim.AdamW, that a
wrong weight-decay coefficient cannot hide inside the tolerance, and the float32 error of the two-pass LayerNorm that sets its tolerance).

Hyper-parameters cross the C ABI as fp32, so the float64 references use the fp32-rounded values (`_f32`): 1 - b2 differs by 1e-5 relative
between float64(0.999...) and the fp32 number the kernel receives, which is the operation's input, not its error.
"""
import functools
import math

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
F64 = torch.float64
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    from lmrl_gym_amd import _lib
    return _lib.require_gpu()


def _f32(x) -> float:
    return float(np.float32(x))


def _close(got, exp, rtol=1e-4, atol=None, name=""):
    """tests/test_gpu_train.py's comparison: |got - exp| <= atol + rtol |exp|, atol = rtol x the largest reference entry by default"""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    atol = atol if atol is not None else rtol * max(float(np.abs(exp).max()), 1e-12)
    np.testing.assert_allclose(got, exp, rtol=rtol, atol=atol, err_msg=name)


def _within(got, exp, frac=1e-5, scale=1.0, name=""):
    """max |got - exp| <= frac x scale x (largest |exp|); prints the figure before asserting.  NaN anywhere fails."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    tol = frac * scale * max(float(np.abs(exp).max()), 1e-30)
    err = float(np.abs(got - exp).max()) if got.size else 0.0
    print(f"{name}: max err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, f"{name}: max err {err:.3e} > {tol:.3e}"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# =================================================================================================== 1. arena AdamW
LR, B1, B2, EPS = _f32(1e-2), _f32(0.9), _f32(0.95), _f32(1e-8)
WD_CYCLE = (0.0, 0.5, 0.1)
ADAMW_TOL = 1e-5               # of the tensor's largest entry: the project's AdamW tolerance (test_train_ops_vs_autograd)
LAYOUT_A = [1, 2, 5, 4093, 4096, 4099, 12288, 12295]


def _cycle_wds(nseg):
    return [WD_CYCLE[i % 3] for i in range(nseg)]


@functools.lru_cache(maxsize=None)
def _model_layout():
    """Segment ends of a parameter arena with a real model's tensors: the ILQL V head (it ends in a Dense(1) whose bias is ONE element, so every
    tensor behind it starts off the 16-byte grid), the two Q heads, then a 1-layer d = 128 GPT2F32 in its gradient order — and the (ends,
    coefficients) `AdamW.__init__` derives from it with the heads' no-decay rule for biases and the model's for biases / LayerNorm."""
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, AdamW, GradArena
    cfg = GPT2Config(1, 2, 128, 512, 211, 32)
    cpu = torch.device("cpu")
    base = GPT2F32(init_hf_style_state_dict(cfg, seed=1), cfg.n_head, device=cpu)
    params = {}
    for head, dout in (("v", 1), ("q1", cfg.vocab), ("q2", cfg.vocab)):
        params[f"{head}.dense1.kernel"] = torch.zeros(128, 256); params[f"{head}.dense1.bias"] = torch.zeros(256)
        params[f"{head}.dense2.kernel"] = torch.zeros(256, dout); params[f"{head}.dense2.bias"] = torch.zeros(dout)
    for k in base.grad_order():
        params[k] = base.p[k]
    arena = GradArena.of_values(params)
    opt = AdamW(arena, LR, b1=B1, b2=B2, eps=EPS, weight_decay=0.5)
    ends, wds = opt._seg_end.tolist(), [float(w) for w in opt._seg_wd.tolist()]
    assert arena.order["v.dense2.bias"] == (128 * 256 + 256 + 256, 1) and any(e % 4 for e in ends)
    return {k: tuple(v.shape) for k, v in params.items()}, ends, wds


def _adamw_layout(name):
    """-> (n, segment ends, per-segment coefficients)"""
    if name == "A":
        return LAYOUT_A[-1], LAYOUT_A, _cycle_wds(len(LAYOUT_A))
    if name.startswith("single"):
        n = int(name[6:])
        return n, [n], [0.5]
    shapes, ends, wds = _model_layout()
    return ends[-1], ends, (_cycle_wds(len(ends)) if name == "model_cycle" else wds)


@functools.lru_cache(maxsize=None)
def _adamw_inputs(name):
    """(p0, tgt0, [g1, g2, g3]) as fp32 numpy; |p| in [0.5, 1.5] so that a wrong decay coefficient moves p by >= lr x 0.1 x 0.5 per step"""
    n = _adamw_layout(name)[0]
    rng = np.random.RandomState(len(name) * 1000 + n % 997)
    p0 = (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    t0 = (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    return p0, t0, gs


def _adamw_ref(p0, t0, gs, ends, wds, alpha=None, lr=LR, b1=B1, b2=B2, eps=EPS):
    """float64, per element: m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr ((m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps) + wd_seg p) ;
    tgt = alpha p_new + (1-alpha) tgt.  -> per step (p, m, v, tgt)"""
    wd = np.repeat(np.asarray([_f32(w) for w in wds], dtype=np.float64), np.diff([0] + list(ends)))
    p, tgt = p0.astype(np.float64), t0.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    a = None if alpha is None else _f32(alpha)
    out = []
    for t, g in enumerate(gs, 1):
        g = g.astype(np.float64)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr * ((m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps) + wd * p)
        if a is not None:
            tgt = a * p + (1 - a) * tgt
        out.append((p.copy(), m.copy(), v.copy(), tgt.copy()))
    return out


def test_adamw_reference_equals_torch_adamw():
    """the float64 restatement == torch.optim.AdamW (decoupled decay == optax.adamw) with one parameter group per segment, to 1e-12"""
    n, ends, wds = _adamw_layout("A")
    p0, t0, gs = _adamw_inputs("A")
    ref = _adamw_ref(p0, t0, gs, ends, wds)
    starts = [0] + ends[:-1]
    segs = [torch.from_numpy(p0[a:b].astype(np.float64)).requires_grad_(True) for a, b in zip(starts, ends)]
    opt = torch.optim.AdamW([dict(params=[s], weight_decay=_f32(w)) for s, w in zip(segs, wds)], lr=LR, betas=(B1, B2), eps=EPS)
    for t, g in enumerate(gs):
        for s, a, b in zip(segs, starts, ends):
            s.grad = torch.from_numpy(g[a:b].astype(np.float64))
        opt.step()
        p = torch.cat([s.detach() for s in segs]).numpy()
        m = torch.cat([opt.state[s]["exp_avg"] for s in segs]).numpy()
        v = torch.cat([opt.state[s]["exp_avg_sq"] for s in segs]).numpy()
        for got, exp in zip((p, m, v), ref[t]):
            assert float(np.abs(got - exp).max()) <= 1e-12 * max(1.0, float(np.abs(exp).max()))


@pytest.mark.parametrize("name", ["A", "model_cycle"])
def test_adamw_wrong_neighbour_coefficient_cannot_hide(name):
    """A condition on the reference alone: with each segment's coefficient replaced by its neighbour's (either side), every element within 4
    of a segment boundary moves away from the true reference by more than 10x the tolerance the GPU tests use, at every step."""
    n, ends, wds = _adamw_layout(name)
    p0, t0, gs = _adamw_inputs(name)
    true = _adamw_ref(p0, t0, gs, ends, wds, alpha=0.5)
    near = np.zeros(n, dtype=bool)
    for e in ends[:-1]:
        near[max(0, e - 4):min(n, e + 4)] = True
    assert near.any()
    for shift in (1, -1):                 # every segment takes its left (right) neighbour's coefficient; the end segments their only neighbour's
        nb = [wds[min(max(s - shift, 0), len(wds) - 1)] for s in range(len(wds))]
        nb[0 if shift == 1 else -1] = wds[1 if shift == 1 else -2]
        assert all(a != b for a, b in zip(nb, wds))
        wrong = _adamw_ref(p0, t0, gs, ends, nb, alpha=0.5)
        for t in range(3):
            for which in (0, 3):          # parameters and the Polyak target (m and v do not depend on the coefficient)
                tol = ADAMW_TOL * float(np.abs(true[t][which]).max())
                diff = np.abs(wrong[t][which] - true[t][which])[near]
                assert float(diff.min()) > 10 * tol, (name, shift, t, which, float(diff.min()), tol)


def _guarded(dev, arr, sentinel=-7.25):
    """device copy of `arr` followed by 8 sentinel floats (16-byte aligned start) -> (view of the n elements, whole buffer)"""
    n = arr.shape[0]
    buf = torch.full(((n + 3) // 4 * 4 + 8,), sentinel, dtype=torch.float32, device=dev)
    buf[:n] = torch.from_numpy(arr).to(dev)
    return buf[:n], buf


def _adamw_check_step(name, step, state, bufs, ref_t, sentinel=-7.25):
    for label, view, exp in zip("pmvt", state, ref_t):
        if view is not None:
            _within(view.cpu().numpy(), exp, ADAMW_TOL, name=f"{name} step {step} {label}")
    for b, view in bufs:
        assert bool((b[view.shape[0]:] == sentinel).all()), "write past the end of the arena"


@gpu
@pytest.mark.parametrize("alpha", [None, 0.005, 0.5])
@pytest.mark.parametrize("name", ["A", "single3", "single4", "single4097", "model_cycle"])
def test_adamw_segments_vs_float64(dev, name, alpha):
    """lmrl_adamw_segments_polyak, three consecutive steps with carried m / v, p / m / v / target against float64 after every step"""
    from lmrl_gym_amd.train import ops
    n, ends, wds = _adamw_layout(name)
    p0, t0, gs = _adamw_inputs(name)
    ref = _adamw_ref(p0, t0, gs, ends, wds, alpha=alpha)
    p, pb = _guarded(dev, p0); m, mb = _guarded(dev, np.zeros(n, np.float32)); v, vb = _guarded(dev, np.zeros(n, np.float32))
    tgt, tb = _guarded(dev, t0 if alpha is not None else np.full(n, 123.5, np.float32))
    seg_end = torch.tensor(ends, dtype=torch.int64, device=dev); seg_wd = torch.tensor(wds, dtype=torch.float32, device=dev)
    for t in range(3):
        g, gb = _guarded(dev, gs[t])
        ops.adamw_segments(p, g, m, v, seg_end, seg_wd, LR, B1, B2, EPS, t + 1, target=tgt if alpha is not None else None,
                           alpha=alpha if alpha is not None else 0.0)
        _adamw_check_step(name, t + 1, (p, m, v, tgt if alpha is not None else None), [(pb, p), (mb, m), (vb, v), (tb, tgt)], ref[t])
        assert torch.equal(g.cpu(), torch.from_numpy(gs[t]))
    if alpha is None:
        assert bool((tgt == 123.5).all())         # no target given: the sentinel-filled buffer is untouched


@gpu
@pytest.mark.parametrize("alpha", [None, 0.005])
def test_adamw_apply_on_model_arena_vs_float64(dev, alpha):
    """The production entry: `AdamW.apply` over a GradArena with the model's own segment table (no decay on biases / LayerNorm) and the
    Polyak target riding in the sweep, three steps against float64."""
    from lmrl_gym_amd.train.gpt2_f32 import AdamW, GradArena
    shapes, ends, wds = _model_layout()
    p0, t0, gs = _adamw_inputs("model_own")
    ref = _adamw_ref(p0, t0, gs, ends, wds, alpha=alpha)
    blank = {k: torch.zeros(s, device=dev) for k, s in shapes.items()}
    params, target, grads = GradArena(blank), GradArena(blank), GradArena(blank)
    params.flat.copy_(torch.from_numpy(p0)); target.flat.copy_(torch.from_numpy(t0))
    nd = lambda k: k.endswith("bias") or ".ln_" in k or k.startswith("ln_f")
    opt = AdamW(params, LR, b1=B1, b2=B2, eps=EPS, weight_decay=0.5, no_decay=nd)
    assert opt._seg_end.tolist() == ends and [float(w) for w in opt._seg_wd.tolist()] == wds
    for t in range(3):
        grads.flat.copy_(torch.from_numpy(gs[t]))
        assert opt.apply(grads, polyak=None if alpha is None else (target, alpha))
        assert opt.polyak_fused == (alpha is not None)
        state = (params.flat, opt.m.flat, opt.v.flat, target.flat if alpha is not None else None)
        _adamw_check_step("model_own", t + 1, state, [], ref[t])
    if alpha is None:
        assert torch.equal(target.flat.cpu(), torch.from_numpy(t0))


@gpu
@pytest.mark.parametrize("name", ["A", "single3", "single4097", "model_cycle"])
def test_adamw_per_segment_vs_float64(dev, name):
    """the same three steps through `lmrl_adamw`, one launch per segment, against the same float64 reference"""
    from lmrl_gym_amd.train import ops
    n, ends, wds = _adamw_layout(name)
    p0, t0, gs = _adamw_inputs(name)
    ref = _adamw_ref(p0, t0, gs, ends, wds)
    p, pb = _guarded(dev, p0); m, mb = _guarded(dev, np.zeros(n, np.float32)); v, vb = _guarded(dev, np.zeros(n, np.float32))
    for t in range(3):
        g = torch.from_numpy(gs[t]).to(dev)
        for a, b, w in zip([0] + ends[:-1], ends, wds):
            ops.adamw(p[a:b], g[a:b], m[a:b], v[a:b], LR, B1, B2, EPS, w, t + 1)
        _adamw_check_step(name + " per segment", t + 1, (p, m, v, None), [(pb, p), (mb, m), (vb, v)], ref[t])


# =================================================================================================== 2. LayerNorm forward family
LN_EPS = 1e-5
LN_ROWS = (1, 5, 131)
LN_VEC_D = (256, 512, 768, 1024, 1280)
LN_STRIDED_D = (96, 1600)
# worst float32 two-pass error on the large-mean inputs as measured on the CPU (`_ln_large_measured`, which the GPU tests call and allow 4x of);
# the figures of one such measurement, which test_layernorm_two_pass_f32_error_measured holds the measurement to
LN_LARGE_RECORDED = dict(y=7.57e-5, mean=1.90e-5, rstd=1.26e-7)


@functools.lru_cache(maxsize=None)
def _ln_inputs(d, R, regime, with_resid):
    """fp32 (x, resid or None, gamma, beta).  'unit': N(0, 1) entries.  'large': rows with mean +-150 and std 1 (as
    tests/test_gpu_forward_vs_oracle.py: a variance computed as E[x^2] - mu^2 loses every digit there)."""
    g = torch.Generator().manual_seed(d * 1000 + R * 4 + (2 if regime == "large" else 0) + int(with_resid))
    x = torch.randn(R, d, generator=g)
    resid = torch.randn(R, d, generator=g) if with_resid else None
    if with_resid:
        x, resid = x * 0.7071, resid * 0.7071
    if regime == "large":
        sign = (torch.randint(0, 2, (R, 1), generator=g) * 2 - 1).float()
        x = x + 150.0 * sign
    gam = torch.randn(d, generator=g); bet = torch.randn(d, generator=g)
    return x.contiguous(), resid, gam, bet


@functools.lru_cache(maxsize=None)
def _ln_ref(d, R, regime, with_resid):
    """-> (fp32 x + resid as the kernel must leave it, float64 y, mean, rstd of that sum)"""
    from oracle import gpt2 as O
    x, resid, gam, bet = _ln_inputs(d, R, regime, with_resid)
    xs = x + resid if resid is not None else x
    x64 = xs.double()
    mu = x64.mean(-1)
    rstd = 1.0 / torch.sqrt(((x64 - mu[:, None]) ** 2).mean(-1) + LN_EPS)
    return xs, O.layer_norm(x64, gam.double(), bet.double(), LN_EPS), mu, rstd


def _ln_two_pass_f32(xs, gam, bet, one_pass=False):
    """the kernels' formula in float32 numpy: mu = mean(x), var = mean((x - mu)^2) (one_pass: E[x^2] - mu^2, the form to catch)"""
    x = xs.numpy().astype(np.float32)
    d = np.float32(x.shape[1])
    mu = x.sum(-1, dtype=np.float32) / d
    if one_pass:
        var = (x * x).sum(-1, dtype=np.float32) / d - mu * mu
    else:
        c = x - mu[:, None]
        var = (c * c).sum(-1, dtype=np.float32) / d
    rs = (np.float32(1.0) / np.sqrt(var + np.float32(LN_EPS))).astype(np.float32)
    y = (x - mu[:, None]) * rs[:, None] * gam.numpy() + bet.numpy()
    return y.astype(np.float32), mu, rs


@functools.lru_cache(maxsize=None)
def _ln_large_measured(one_pass=False):
    worst = dict(y=0.0, mean=0.0, rstd=0.0)
    for d in LN_VEC_D + LN_STRIDED_D:
        for R in LN_ROWS:
            for wr in (False, True):
                _, _, gam, bet = _ln_inputs(d, R, "large", wr)
                xs, y64, mu64, rs64 = _ln_ref(d, R, "large", wr)
                y, mu, rs = _ln_two_pass_f32(xs, gam, bet, one_pass)
                with np.errstate(invalid="ignore"):
                    for k, got, exp in (("y", y, y64), ("mean", mu, mu64), ("rstd", rs, rs64)):
                        e = np.abs(got.astype(np.float64) - exp.numpy())
                        worst[k] = max(worst[k], float(np.nan_to_num(e, nan=np.inf).max()))
    return worst


def test_layernorm_two_pass_f32_error_measured():
    """The large-mean tolerance is measured, not guessed: the two-pass formula in float32 numpy against float64 on the very inputs the GPU
    tests use (rows with mean +-150, std 1; every d and row count; with and without the residual).  Measured worst absolute errors:
    y 7.57e-5, mean 1.90e-5 (1.25 ulp of 150), rstd 1.26e-7 (1 ulp of 1) — LN_LARGE_RECORDED; the GPU tests allow 4x the measurement.
    The one-pass form E[x^2] - mu^2 in float32 misses that bound by orders of magnitude (y 2.8e-2, rstd 4.3e-3 measured), so the bound catches it."""
    got = _ln_large_measured()
    print("float32 two-pass LayerNorm, worst error vs float64:", got)
    for k, rec in LN_LARGE_RECORDED.items():
        assert 0.75 * rec <= got[k] <= 1.25 * rec, (k, got[k], rec)
    bad = _ln_large_measured(one_pass=True)
    print("float32 one-pass (E[x^2] - mu^2) form:", bad)
    assert bad["y"] > 40 * got["y"] and bad["rstd"] > 40 * got["rstd"]


def _ln_check(regime, got_y, got_mean, got_rstd, ref, name):
    xs, y64, mu64, rs64 = ref
    if regime == "unit":
        if got_y is not None:
            _close(got_y.cpu(), y64, rtol=1e-5, name=name + " y")
        # the mean of N(0, 1) entries is a sum that nearly cancels (|mu| ~ d^-1/2, 1.8e-4 on one of these rows): its fp32 error scales with the
        # entries, so the 1e-5 applies to their mean magnitude, not to the largest mean
        _close(got_mean.cpu(), mu64, rtol=1e-5, atol=1e-5 * float(xs.abs().mean()), name=name + " mean")
        _close(got_rstd.cpu(), rs64, rtol=1e-5, name=name + " rstd")
        return
    for k, got, exp in (("y", got_y, y64), ("mean", got_mean, mu64), ("rstd", got_rstd, rs64)):
        if got is None:
            continue
        err = float((got.cpu().double() - exp).abs().max())
        tol = 4 * _ln_large_measured()[k]
        print(f"{name} {k}: max err {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, (name, k, err, tol)


def _ln_run(dev, d, R, regime, with_resid, staged=False):
    from lmrl_gym_amd.train import ops
    x, resid, gam, bet = _ln_inputs(d, R, regime, with_resid)
    ref = _ln_ref(d, R, regime, with_resid)
    gd, bd = gam.to(dev), bet.to(dev)
    rd = resid.to(dev) if resid is not None else None
    ldb = d + 8
    name = f"d={d} R={R} {regime} resid={with_resid} staged={staged}"

    def run(with_y):
        xd = x.to(dev).clone()
        y = torch.full((R, d), 9.0, device=dev) if with_y else None
        mean, rstd = torch.full((R,), 9.0, device=dev), torch.full((R,), 9.0, device=dev)
        yb = torch.full((R, ldb), 3.0, dtype=BF16, device=dev)
        if staged:
            ops.layernorm_fwd_staged(xd, gd, bd, y, mean, rstd, yb, ldb, R, d, LN_EPS)
        else:
            ops.layernorm_add_fwd(xd, rd, gd, bd, y, mean, rstd, yb, ldb, R, d, LN_EPS)
        return xd, y, mean, rstd, yb

    xd, y, mean, rstd, yb = run(True)
    assert _same_bits(xd, ref[0]), name + ": x must be the fp32 sum x + resid"
    _ln_check(regime, y, mean, rstd, ref, name)
    assert _same_bits(yb[:, :d], y.to(BF16)), name + ": bf16 copy"
    assert bool((yb[:, d:] == 3.0).all()), name + ": pad columns written"
    xd2, _, mean2, rstd2, yb2 = run(False)                                  # bf16 copy only
    assert _same_bits(xd2, ref[0]) and _same_bits(yb2, yb) and _same_bits(mean2, mean) and _same_bits(rstd2, rstd), name + ": y = None form"
    if not staged:
        ops._L().lmrl_train_ops_set_variant(1)                              # the strided kernel at every width
        try:
            xd3, y3, mean3, rstd3, yb3 = run(True)
        finally:
            ops._L().lmrl_train_ops_set_variant(0)
        assert _same_bits(xd3, ref[0])
        _ln_check(regime, y3, mean3, rstd3, ref, name + " variant 1")
        assert _same_bits(yb3[:, :d], y3.to(BF16)) and bool((yb3[:, d:] == 3.0).all())


@gpu
@pytest.mark.parametrize("regime", ["unit", "large"])
@pytest.mark.parametrize("d", LN_VEC_D + LN_STRIDED_D)
def test_layernorm_add_fwd_vs_float64(dev, d, regime):
    """lmrl_layernorm_add_fwd: ln_fwd_vec_kernel<1..5> at d = 256..1280, the axpby + strided kernel at d = 96 / 1600; rows 1 / 5 / 131 with and
    without the residual.  Large-mean tolerance: 4x the measured float32 two-pass error (test_layernorm_two_pass_f32_error_measured)."""
    for R in LN_ROWS:
        for with_resid in (False, True):
            _ln_run(dev, d, R, regime, with_resid)


@gpu
@pytest.mark.parametrize("regime", ["unit", "large"])
@pytest.mark.parametrize("d", [96, 768])
def test_layernorm_fwd_staged_vs_float64(dev, d, regime):
    for R in LN_ROWS:
        _ln_run(dev, d, R, regime, False, staged=True)


def _split3_expect(y):
    """[hi | lo | hi] of fp32 y [R, n]: hi = bf16(y), lo = bf16(y - hi)"""
    hi = y.to(BF16)
    lo = (y - hi.float()).to(BF16)
    return torch.cat([hi, lo, hi], dim=1)


@gpu
@pytest.mark.parametrize("with_resid", [False, True])
@pytest.mark.parametrize("d", [256, 768, 1280])
def test_layernorm_add_fwd_split3_bits(dev, d, with_resid):
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.train import ops
    R = 5
    x, resid, gam, bet = _ln_inputs(d, R, "unit", with_resid)
    gd, bd = gam.to(dev), bet.to(dev)
    rd = resid.to(dev) if resid is not None else None
    xd = x.to(dev).clone(); y = torch.empty(R, d, device=dev); mean, rstd = torch.empty(R, device=dev), torch.empty(R, device=dev)
    ops.layernorm_add_fwd(xd, rd, gd, bd, y, mean, rstd, None, 0, R, d, LN_EPS)
    _ln_check("unit", y, mean, rstd, _ln_ref(d, R, "unit", with_resid), f"split3 base d={d}")
    xs = x.to(dev).clone(); mean2, rstd2 = torch.empty(R, device=dev), torch.empty(R, device=dev)
    out = torch.full((R + 1, 3 * d), 3.0, dtype=BF16, device=dev)
    _lib.check(ops._L().lmrl_layernorm_add_fwd_split3(xs.data_ptr(), _lib.ptr(rd), gd.data_ptr(), bd.data_ptr(), mean2.data_ptr(), rstd2.data_ptr(),
                                                       out.data_ptr(), R, d, LN_EPS, _lib.stream_ptr()), "lmrl_layernorm_add_fwd_split3")
    assert _same_bits(out[:R], _split3_expect(y)) and bool((out[R] == 3.0).all())
    assert _same_bits(out[:R, :d], out[:R, 2 * d:])
    assert _same_bits(xs, xd) and _same_bits(mean2, mean) and _same_bits(rstd2, rstd)


@gpu
@pytest.mark.parametrize("rows,cols", [(3, 4), (7, 3072)])
def test_gelu_split3_bits(dev, rows, cols):
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.train import ops
    from oracle import gpt2 as O
    g = torch.Generator().manual_seed(rows * cols)
    x = torch.randn(rows, cols, generator=g) * 2
    xd = x.to(dev); y = torch.empty_like(xd)
    ops.gelu_fwd(xd, y)
    _close(y.cpu(), O.gelu_new(x.double()), rtol=1e-5)
    out = torch.full((rows + 1, 3 * cols), 3.0, dtype=BF16, device=dev)
    _lib.check(ops._L().lmrl_gelu_split3(xd.data_ptr(), rows, cols, out.data_ptr(), _lib.stream_ptr()), "lmrl_gelu_split3")
    assert _same_bits(out[:rows], _split3_expect(y)) and bool((out[rows] == 3.0).all())


# =================================================================================================== 3. LayerNorm backward
@functools.lru_cache(maxsize=1)
def _ln_bwd_case(R, d):
    from oracle import gpt2 as O
    g = torch.Generator().manual_seed(R * 7 + d)
    x = torch.randn(R, d, generator=g) * 2 + 0.5; gam = torch.randn(d, generator=g); bet = torch.randn(d, generator=g)
    dy = torch.randn(R, d, generator=g)
    xr = x.double().requires_grad_(True); gr = gam.double().requires_grad_(True); br = bet.double().requires_grad_(True)
    O.layer_norm(xr, gr, br, LN_EPS).backward(dy.double())
    mu = x.double().mean(-1, keepdim=True)
    xhat = (x.double() - mu) / torch.sqrt(((x.double() - mu) ** 2).mean(-1, keepdim=True) + LN_EPS)
    return x, gam, bet, dy, xr.grad, gr.grad, br.grad, dy.double() * xhat


@gpu
@pytest.mark.parametrize("form", ["vector", "pitch66", "variant2"])
@pytest.mark.parametrize("d,R", [(d, R) for d in (256, 768, 1024, 1280) for R in (37, 2051)])
def test_layernorm_bwd_fused_forms_vs_autograd(dev, d, R, form):
    """lmrl_layernorm_bwd_fused at d = 256 / 1280 (no test ran them) and in its non-vector form ln_bwd_fused_kernel<4|12|16|20>: taken with a bf16
    pitch that is no multiple of 4 (d + 66) or with variant 2.  R = 2051: 8 rows per workgroup and a ragged last slab of 3 rows.  dx, dgamma,
    dbeta against float64 autograd at the tolerances of test_layernorm_bwd_fused_vs_autograd; accumulate flags on and off; two runs bit-identical."""
    from lmrl_gym_amd.train import ops
    x, gam, bet, dy, dx_ref, dg_ref, db_ref, _ = _ln_bwd_case(R, d)
    xd, gd, bd, dyd = x.to(dev), gam.to(dev), bet.to(dev), dy.to(dev)
    yd, mean, rstd = torch.empty_like(xd), torch.empty(R, device=dev), torch.empty(R, device=dev)
    ops.layernorm_fwd(xd, gd, bd, yd, mean, rstd, R, d, LN_EPS)
    ws = torch.empty(ops.layernorm_bwd_fused_ws_floats(R, d), device=dev)
    ldb = d + 66 if form == "pitch66" else d + 64
    at = 1e-4 * math.sqrt(R)
    ops._L().lmrl_train_ops_set_variant(2 if form == "variant2" else 0)
    try:
        outs = []
        for rep in range(2):
            dxd = torch.full_like(xd, 3.0); dg = torch.full((d,), 2.0, device=dev); db = torch.full((d,), -1.0, device=dev)
            dxb = torch.full((R, ldb), 5.0, dtype=BF16, device=dev)
            ops.layernorm_bwd_fused(dyd, xd, gd, mean, rstd, dxd, dg, db, R, d, True, True, ws, dxb, ldb)      # everything accumulates
            assert _same_bits(dxb[:, :d], dxd.to(BF16)) and bool((dxb[:, d:] == 5.0).all())
            outs.append((dxd.clone(), dg.clone(), db.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*outs))
        dxd, dg, db = outs[0]
        _close(dxd.cpu() - 3.0, dx_ref, rtol=2e-5, atol=2e-5, name="dx (accumulated)")
        _close(dg.cpu() - 2.0, dg_ref, rtol=2e-5, atol=at, name="dgamma (accumulated)")
        _close(db.cpu() + 1.0, db_ref, rtol=2e-5, atol=at, name="dbeta (accumulated)")
        dxd = torch.full_like(xd, 7.0); dg = torch.full((d,), 7.0, device=dev); db = torch.full((d,), 7.0, device=dev)
        ops.layernorm_bwd_fused(dyd, xd, gd, mean, rstd, dxd, dg, db, R, d, False, False, ws)                  # overwrite, no bf16 copy
        _close(dxd.cpu(), dx_ref, rtol=2e-5, atol=2e-5, name="dx")
        _close(dg.cpu(), dg_ref, rtol=2e-5, atol=at, name="dgamma"); _close(db.cpu(), db_ref, rtol=2e-5, atol=at, name="dbeta")
    finally:
        ops._L().lmrl_train_ops_set_variant(0)


@gpu
@pytest.mark.parametrize("accumulate", [False, True])
def test_layernorm_bwd_unfused_d512(dev, accumulate):
    from lmrl_gym_amd.train import ops
    R, d = 37, 512
    x, gam, bet, dy, dx_ref, _, _, dyxh_ref = _ln_bwd_case(R, d)
    xd, gd, bd, dyd = x.to(dev), gam.to(dev), bet.to(dev), dy.to(dev)
    yd, mean, rstd = torch.empty_like(xd), torch.empty(R, device=dev), torch.empty(R, device=dev)
    ops.layernorm_fwd(xd, gd, bd, yd, mean, rstd, R, d, LN_EPS)
    base = 3.0 if accumulate else 0.0
    dxd, tmp = torch.full_like(xd, 3.0), torch.full_like(xd, 9.0)
    ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dxd, tmp, R, d, accumulate)
    _close(dxd.cpu() - base, dx_ref, rtol=1e-5, name="dx"); _close(tmp.cpu(), dyxh_ref, rtol=1e-5, name="dy*xhat")
    dx2 = torch.full_like(xd, 3.0)
    ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dx2, None, R, d, accumulate)                                   # without the dy * xhat output
    assert torch.equal(dx2, dxd)


# =================================================================================================== 4. causal softmax
def _softmax_mask(kind, B, T, g):
    if kind == "none":
        return None
    km = torch.ones(B, T, dtype=torch.uint8)
    k = max(1, T // 3)
    if kind == "right":
        km[B - 1, T - k:] = 0
    elif kind == "left":
        km[B - 1, :k] = 0                       # query rows r < k of that batch entry have no valid key
    else:
        km = (torch.rand(B, T, generator=g) < 0.7).to(torch.uint8)
        km[:, 0] = 0                            # row 0 of every (b, h) has no valid key
    return km


def _softmax_ref(S, km, H):
    """float64: P[r][c] = softmax over c <= r with km[b][c] != 0, 0 elsewhere; a row with no valid key is all zeros -> (P, valid [BH, T, T])"""
    BH, T, _ = S.shape
    valid = torch.tril(torch.ones(T, T, dtype=torch.bool))[None].expand(BH, T, T)
    if km is not None:
        valid = valid & km.bool().repeat_interleave(H, 0)[:, None, :]
    Sm = S.double().masked_fill(~valid, float("-inf"))
    mx = Sm.amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    E = torch.exp(Sm - mx)
    tot = E.sum(-1, keepdim=True)
    return E / torch.where(tot == 0, torch.ones_like(tot), tot), valid


@gpu
@pytest.mark.parametrize("kind", ["none", "right", "left", "holes"])
@pytest.mark.parametrize("B,H,T", [(2, 3, 1), (2, 3, 63), (2, 2, 64), (2, 3, 65), (1, 3, 65), (2, 3, 130), (2, 3, 257)])
def test_softmax_causal_fwd_bwd_vs_float64(dev, B, H, T, kind):
    """more than one 64-lane sweep (T > 64), row counts that are no multiple of 4, rows without a valid key (exact zeros, forward and
    backward), and the in-place forward (same bits as out of place)"""
    from lmrl_gym_amd.train import ops
    g = torch.Generator().manual_seed(T * 10 + B)
    S = torch.randn(B * H, T, T, generator=g) * 2; dP = torch.randn(B * H, T, T, generator=g)
    km = _softmax_mask(kind, B, T, g)
    P, valid = _softmax_ref(S, km, H)
    dS = P * (dP.double() - (dP.double() * P).sum(-1, keepdim=True))
    empty = ~valid.any(-1)                                                   # [BH, T] rows with no valid key
    assert kind in ("none", "right") or bool(empty.any())
    Sd = S.to(dev); Pd = torch.full_like(Sd, 9.0)
    kmd = km.to(dev) if km is not None else None
    ops.softmax_causal_fwd(Sd, kmd, Pd, B, H, T)
    _close(Pd.cpu(), P, rtol=1e-5, name="P")
    assert bool((Pd.cpu()[~valid] == 0).all()) and bool((Pd.cpu()[empty] == 0).all())
    Si = S.to(dev).clone()
    ops.softmax_causal_fwd(Si, kmd, Si, B, H, T)
    assert _same_bits(Si, Pd), "in place"
    dPd = dP.to(dev).clone()
    ops.softmax_bwd(Pd, dPd, B * H * T, T)
    _close(dPd.cpu(), dS, rtol=1e-5, name="dS")
    assert bool((dPd.cpu()[empty] == 0).all()) and bool((dPd.cpu()[~valid] == 0).all())


# =================================================================================================== 5. log-softmax gather / CE backward
LSE_SHAPES = [(1003, 1003), (1003, 1005), (3, 3), (1, 1), (200, 203), (50257, 50257)]
LSE_ROWS = 5


def _lse_logits(V, ld, regime, g):
    """fp32 [R, ld] logits.  'normal': N(0, 3^2).  'wide:<where>': entries in +-80 with the row maximum (+80, a few entries within 2 of it
    elsewhere) at the first column (the scalar head of an unaligned row), the middle (vector body) or the last column (scalar tail)."""
    R = LSE_ROWS
    if regime == "normal":
        return torch.randn(R, ld, generator=g) * 3
    lg = torch.rand(R, ld, generator=g) * 158 - 80          # [-80, 78)
    at = dict(first=0, middle=V // 2, last=V - 1)[regime.split(":")[1]]
    lg[:, at] = 80.0
    return lg


def _ce_bwd_f32(logits, lse64, tc, cc, cg):
    """The CE backward's formula in float32 numpy with the best lse fp32 can carry (the float64 one, rounded): coef_ce exp(x - lse), plus
    coef_gather - coef_ce at the target.  Its distance from float64 is the error of the arithmetic itself: lse ~ 80 is known to 3.8e-6 at
    best, so a probability of 1 - 2.9e-6 comes out as 1 and coef_ce (p - 1) as 0."""
    x = logits.numpy().astype(np.float32)
    l = lse64.numpy().astype(np.float32)
    R = x.shape[0]
    c = cc.numpy().astype(np.float32) if cc is not None else np.zeros(R, np.float32)
    gth = cg.numpy().astype(np.float32) if cg is not None else np.zeros(R, np.float32)
    out = (c[:, None] * np.exp(x - l[:, None], dtype=np.float32)).astype(np.float32)
    out[np.arange(R), tc.numpy()] += gth - c
    return out.astype(np.float64)


@gpu
@pytest.mark.parametrize("regime", ["normal", "wide:first", "wide:middle", "wide:last"])
@pytest.mark.parametrize("V,ld", LSE_SHAPES)
def test_lse_gather_and_ce_bwd_vs_float64(dev, V, ld, regime):
    """Rows that start at each 16-byte phase (ld odd): the unaligned scalar head, the float4 body, the scalar tail; V < 256 (threads that
    carry -inf into the merge), V < 4 (no vector body at all); the running rescale with the maximum met early, in the body and last.  lse and
    logprob to 1e-5 of their largest entry, as test_train_ops_vs_autograd; the target logit is a copy (exact).
    CE backward: 1e-5 of the largest entry of the float64 autograd gradient, and no less than 4x the error of the same formula in float32 numpy
    given the correctly rounded lse (`_ce_bwd_f32`): at V = 3 with the maximum 80 in the first column a row's gradient is coef_ce (p - 1) with
    p = 1 - 2.9e-6, which fp32 cannot form from lse = 80 + 2.9e-6 (restatement error 2.9e-6 against 1e-5 x 0.24 = 2.4e-6)."""
    from lmrl_gym_amd.train import ops
    R = LSE_ROWS
    g = torch.Generator().manual_seed(V + ld + len(regime))
    lg = _lse_logits(V, ld, regime, g)
    tgt = torch.randint(0, V, (R,), generator=g).to(torch.int32)
    tgt[1], tgt[3] = -3, V + 5                                                # clamp to 0 and V - 1
    tc = tgt.long().clamp(0, V - 1)
    cce = torch.randn(R, generator=g); cga = torch.randn(R, generator=g)
    lr = lg[:, :V].double().requires_grad_(True)
    lse_ref = torch.logsumexp(lr, -1)
    tl_ref = lr.gather(1, tc[:, None])[:, 0]
    lp_ref = tl_ref - lse_ref
    lgd = lg.to(dev).contiguous()
    phases = {(lgd.data_ptr() + 4 * r * ld) % 16 for r in range(R)}
    assert phases == {0, 4, 8, 12}, phases
    td = tgt.to(dev)
    lpd, lsed, tld = (torch.full((R,), 9.0, device=dev) for _ in range(3))
    ops.lse_gather(lgd, ld, V, td, R, logprob=lpd, lse=lsed, target_logit=tld)
    assert torch.equal(lgd.cpu(), lg)
    _within(lsed.cpu(), lse_ref.detach(), 1e-5, name="lse")
    if V > 1:
        _within(lpd.cpu(), lp_ref.detach(), 1e-5, name="logprob")
    else:
        assert float(lpd.abs().max()) <= 1e-5
    assert torch.equal(tld.cpu(), lg[:, :V].gather(1, tc[:, None])[:, 0])
    for only in ("logprob", "lse", "target_logit"):                           # every output pointer is optional
        out = torch.full((R,), 9.0, device=dev)
        ops.lse_gather(lgd, ld, V, td, R, **{only: out})
        assert torch.equal(out, dict(logprob=lpd, lse=lsed, target_logit=tld)[only]), only
    # CE backward over the logits, in place, with the kernel's own lse (as the train steps call it)
    for ce_kind, with_gather in (("nonzero", True), ("nonzero", False), ("zero", True), ("none", True)):
        cc = dict(nonzero=cce, zero=torch.zeros(R), none=None)[ce_kind]
        cg = cga if with_gather else None
        lr.grad = None
        loss = (lr * 0).sum()
        if cc is not None:
            loss = loss + ((-lp_ref) * cc.double()).sum()
        if cg is not None:
            loss = loss + (tl_ref * cg.double()).sum()
        loss.backward(retain_graph=True)
        buf = lg.to(dev).contiguous()
        if ld > V:
            buf[:, V:] = 5.0
        ops.ce_bwd(buf, ld, V, lsed, td, cc.to(dev) if cc is not None else None, cg.to(dev) if cg is not None else None, R)
        got = buf.cpu()
        f32_err = float(np.abs(_ce_bwd_f32(lg[:, :V], lse_ref.detach(), tc, cc, cg) - lr.grad.numpy()).max())
        tol = max(1e-5 * float(lr.grad.abs().max()), 4 * f32_err)
        err = float((got[:, :V].double() - lr.grad).abs().max())
        print(f"ce_bwd {ce_kind} gather={with_gather}: max err {err:.3e} (tolerance {tol:.3e}, float32 restatement {f32_err:.3e})")
        assert err <= tol, (ce_kind, with_gather, err, tol)
        assert ld == V or float(got[:, V:].abs().max()) == 0.0, "pad columns must be zeroed"


@gpu
def test_lse_gather_with_masked_logits(dev):
    """Logits of -inf (a masked vocabulary entry; `ilql_loss` / `mc_loss` take caller-supplied logits with the reference's signature): a thread
    that meets -inf before any finite value must not form exp(-inf - -inf).  Runs of -inf across whole float4 groups, the scalar head and the
    tail; the target on a masked entry gives logprob -inf; the CE backward gives exact zeros there."""
    from lmrl_gym_amd.train import ops
    R, V = LSE_ROWS, 1003
    g = torch.Generator().manual_seed(77)
    lg = torch.randn(R, V, generator=g) * 3
    ninf = float("-inf")
    lg[0, :520] = ninf; lg[1, 500:] = ninf; lg[2, ::2] = ninf; lg[3, :] = ninf; lg[3, 700] = 1.5; lg[4, :3] = ninf; lg[4, -3:] = ninf
    tgt = torch.tensor([600, 100, 1, 700, 0], dtype=torch.int32)             # row 4: the target itself is masked
    lse_ref = torch.logsumexp(lg.double(), -1)
    lp_ref = lg.double().gather(1, tgt.long()[:, None])[:, 0] - lse_ref
    lgd, td = lg.to(dev), tgt.to(dev)
    lpd, lsed = torch.empty(R, device=dev), torch.empty(R, device=dev)
    ops.lse_gather(lgd, V, V, td, R, logprob=lpd, lse=lsed)
    _within(lsed.cpu(), lse_ref, 1e-5, name="lse with -inf logits")
    assert float(lpd[4]) == ninf
    _within(lpd.cpu()[:4], lp_ref[:4], 1e-5, name="logprob with -inf logits")
    cce = torch.tensor([1.0, -0.5, 2.0, 0.3, 0.0])
    ops.ce_bwd(lgd, V, V, lsed, td, cce.to(dev), None, R)
    ref = cce.double()[:, None] * (torch.softmax(lg.double(), -1) - torch.nn.functional.one_hot(tgt.long(), V).double())
    _within(lgd.cpu(), ref, 1e-5, name="ce_bwd with -inf logits")
    assert bool((lgd.cpu()[torch.isinf(lg) & (torch.arange(V)[None] != tgt.long()[:, None])] == 0).all())


# =================================================================================================== 6. column sums
@gpu
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 200, 1000])
def test_colsum_and_weighted_vs_float64(dev, rows):
    """rows >= 64: slabs of several rows, the 8-way unrolled body and its tail; ld = cols + 3; weights at stride 1 and 5; accumulate on and
    off; two runs bit-identical.  Tolerance 1e-5 of the largest entry, x sqrt(rows / 64) for rows > 64."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.train import ops
    scale = math.sqrt(rows / 64) if rows > 64 else 1.0
    for cols in (1, 257, 768):
        ld = cols + 3
        g = torch.Generator().manual_seed(rows * 1000 + cols)
        x = torch.randn(rows, ld, generator=g) + 0.5
        init = torch.randn(cols, generator=g)
        xd = x.to(dev); ws = torch.empty(64 * cols, device=dev)
        for ldw in (0, 1, 5):                                                  # 0: the unweighted lmrl_colsum
            w = torch.randn(rows * max(ldw, 1), generator=g) + 0.5
            wd = w.to(dev)
            wr = w[::ldw].double() if ldw else torch.ones(rows, dtype=F64)
            ref = (x[:, :cols].double() * wr[:, None]).sum(0)
            for acc in (False, True):
                outs = []
                for rep in range(2):
                    out = init.to(dev).clone()
                    if ldw:
                        _lib.check(ops._L().lmrl_colsum_weighted(xd.data_ptr(), rows, cols, ld, wd.data_ptr(), ldw, out.data_ptr(), int(acc), ws.data_ptr(),
                                                                 _lib.stream_ptr()), "lmrl_colsum_weighted")
                    else:
                        ops.colsum(xd, rows, cols, ld, out, acc, ws)
                    outs.append(out.cpu())
                assert torch.equal(outs[0], outs[1])
                _within(outs[0], ref + (init.double() if acc else 0.0), 1e-5, scale, name=f"colsum rows={rows} cols={cols} ldw={ldw} acc={acc}")


# =================================================================================================== 7. elementwise, gather / scatter, embedding
@gpu
def test_elementwise_past_the_grid_cap_vs_float64(dev):
    """n = 4096 x 256 + 257: past ew_grid's cap, so every thread takes the grid-stride loop a second time and the last 257 elements are a
    partial round"""
    from lmrl_gym_amd.train import ops
    from oracle import gpt2 as O
    n = 4096 * 256 + 257
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, generator=g) * 2; dy = torch.randn(n, generator=g); y2 = torch.randn(n, generator=g)
    xd, dyd, y2d = x.to(dev), dy.to(dev), y2.to(dev)
    xr = x.double().requires_grad_(True); O.gelu_new(xr).backward(dy.double())
    out, dxd = torch.full_like(xd, 9.0), torch.full_like(xd, 9.0)
    ops.gelu_fwd(xd, out); ops.gelu_bwd(dyd, xd, dxd)
    _within(out.cpu(), O.gelu_new(x.double()), 1e-5, name="gelu_fwd"); _within(dxd.cpu(), xr.grad, 1e-5, name="gelu_bwd")
    out, dxd = torch.full_like(xd, 9.0), torch.full_like(xd, 9.0)
    ops.relu_fwd(xd, out); ops.relu_bwd(dyd, xd, dxd)
    assert torch.equal(out.cpu(), x.clamp_min(0)) and torch.equal(dxd.cpu(), torch.where(x > 0, dy, torch.zeros_like(dy)))
    out = torch.full_like(xd, 9.0)
    ops.axpby(0.75, xd, -1.5, y2d, out)
    _within(out.cpu(), _f32(0.75) * x.double() - 1.5 * y2.double(), 1e-5, name="axpby")
    out = torch.full_like(xd, 9.0)
    ops.axpby(0.3, xd, 0.0, None, out)                                          # y = None
    _within(out.cpu(), _f32(0.3) * x.double(), 1e-5, name="axpby y=None")
    xi = xd.clone()
    ops.axpby(0.5, xi, 2.0, y2d, xi)                                            # in place on x
    _within(xi.cpu(), 0.5 * x.double() + 2.0 * y2.double(), 1e-5, name="axpby in place (x)")
    yi = y2d.clone()
    ops.axpby(0.5, xd, 2.0, yi, yi)                                             # in place on y
    _within(yi.cpu(), 0.5 * x.double() + 2.0 * y2.double(), 1e-5, name="axpby in place (y)")
    # adamw, three steps
    p0 = (x.numpy() / 2 + np.sign(x.numpy())).astype(np.float32)
    gs = [dy.numpy(), y2.numpy(), (dy.numpy() * y2.numpy()).astype(np.float32)]
    ref = _adamw_ref(p0, p0, gs, [n], [0.1])
    p = torch.from_numpy(p0).to(dev); m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t in range(3):
        ops.adamw(p, torch.from_numpy(gs[t]).to(dev), m, v, LR, B1, B2, EPS, 0.1, t + 1)
    for label, got, exp in zip("pmv", (p, m, v), ref[2]):
        _within(got.cpu().numpy(), exp, ADAMW_TOL, name="adamw " + label)


@gpu
@pytest.mark.parametrize("cols", [4, 7, 12, 100, 3072 + 4])
def test_gelu_staged_tails_vs_float64(dev, cols):
    """gelu_fwd_staged / gelu_bwd_staged: the cols % 8 == 4 tail of the 8-column groups (4, 12, 100, 3076), the scalar path for cols % 4 != 0
    (7: none of the other widths reaches it), and a bf16 pitch that is no multiple of 8.  The bf16 outputs: the forward's equals bf16(y) bit
    for bit; the backward's against float64 within one bf16 rounding (2^-8 relative: half an ulp is 2^-9, the fp32 error in front of the
    rounding can move a value across a tie; plus the fp32 tolerance, 1e-5 of the largest entry)."""
    from lmrl_gym_amd.train import ops
    from oracle import gpt2 as O
    rows = 3
    g = torch.Generator().manual_seed(cols)
    x = torch.randn(rows, cols, generator=g) * 2; dy = torch.randn(rows, cols, generator=g)
    xd, dyd = x.to(dev), dy.to(dev)
    xr = x.double().requires_grad_(True); O.gelu_new(xr).backward(dy.double())
    for ldb in ((cols + 7) // 8 * 8 + 8, cols + 3):
        y = torch.full((rows, cols), 9.0, device=dev); yb = torch.full((rows, ldb), 3.0, dtype=BF16, device=dev)
        ops.gelu_fwd_staged(xd, y, yb, ldb, rows, cols)
        _close(y.cpu(), O.gelu_new(x.double()), rtol=1e-5, name="gelu_fwd_staged y")
        assert _same_bits(yb[:, :cols], y.to(BF16)) and bool((yb[:, cols:] == 3.0).all())
        yb2 = torch.full((rows, ldb), 3.0, dtype=BF16, device=dev)
        ops.gelu_fwd_staged(xd, None, yb2, ldb, rows, cols)
        assert _same_bits(yb2, yb)
    mm = ops.MatmulBF16(dev)
    dst = ops.gelu_bwd_staged(mm, dyd, xd, rows, cols)
    ldb, rd = ops._pitch(cols), ops._padn(rows)
    got = dst[:rd * ldb].view(rd, ldb).float().cpu()
    ref = xr.grad
    assert bool(((got[:rows, :cols].double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-5 * float(ref.abs().max())).all())
    assert float(got[rows:].abs().max()) == 0.0 and float(got[:, cols:].abs().max()) == 0.0          # padding zero-filled


@gpu
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("d", [5, 64, 260])
def test_gather_scatter_rows_exact(dev, d, n):
    """d % 4 != 0 takes the scalar path (5: one partial sweep; 260 is a multiple of 4 past one 256-column sweep)"""
    from lmrl_gym_amd.train import ops
    g = torch.Generator().manual_seed(d * 10 + n)
    src = torch.randn(23, d, generator=g)
    idx = torch.randperm(23, generator=g)[:n].to(torch.int32)
    got = ops.gather_rows(src.to(dev), idx.to(dev), n, d)
    assert torch.equal(got.cpu(), src[idx.long()])
    rows = torch.randn(n, d, generator=g)
    for acc in (False, True):
        dst = src.clone()
        dd = dst.to(dev)
        ops.scatter_rows(rows.to(dev), idx.to(dev), dd, n, d, acc)
        if acc:
            dst[idx.long()] += rows
        else:
            dst[idx.long()] = rows
        assert torch.equal(dd.cpu(), dst)


@gpu
@pytest.mark.parametrize("mode", ["all", "live", "live_next"])
@pytest.mark.parametrize("d", [768, 772, 1280, 1600])
def test_embed_bwd_vs_float64(dev, d, mode):
    """embed_bwd_kernel<12 | 20 | 32>; R = 203 = 7 sequences of 29 with ids from 6 values (two of them outside the vocabulary: no table row),
    so rows that share an index sit more than 64 and more than 128 rows apart and the ballot loop runs over several bases; left-padded `live`
    flags alone (t_row = 0) and with t_row = T (a flag-0 row whose next position is attended is live).  Two runs bit-identical."""
    from lmrl_gym_amd.train import ops
    B, T, vocab = 7, 29, 5
    R = B * T
    g = torch.Generator().manual_seed(d)
    ids = torch.tensor([0, 1, 2, 3, 5, 6])[torch.randint(0, 6, (R,), generator=g)].to(torch.int32)
    pos = torch.arange(T, dtype=torch.int32).repeat(B)
    dx = torch.randn(R, d, generator=g)
    w0 = torch.randn(vocab, d, generator=g); p0 = torch.randn(T, d, generator=g)
    live = torch.ones(B, T, dtype=torch.uint8)
    for b in range(B):
        live[b, :(b * 3) % 11] = 0                                              # left padding of 0..10 positions
    live = live.view(-1)
    if mode == "all":
        eff, lv, t_row = torch.ones(R, dtype=torch.bool), None, 0
    else:
        eff = live.bool().clone()
        t_row = T if mode == "live_next" else 0
        if t_row:
            nxt = torch.zeros(R, dtype=torch.bool)
            nxt[:-1] = live[1:].bool()
            nxt[torch.arange(R) % T == T - 1] = False
            eff |= nxt
            assert int(eff.sum()) > int(live.sum())
        lv = live.to(dev)
    rw = eff & (ids >= 0) & (ids < vocab)
    wref = w0.double().index_add(0, ids.long()[rw], dx.double()[rw])
    pref = p0.double().index_add(0, pos.long()[eff], dx.double()[eff])
    outs = []
    for rep in range(2):
        dw, dp = w0.to(dev).clone(), p0.to(dev).clone()
        ops.embed_bwd(dx.to(dev), ids.to(dev), pos.to(dev), dw, dp, R, d, live=lv, vocab=vocab, t_row=t_row)
        outs.append((dw.cpu(), dp.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _within(outs[0][0], wref, 1e-5, name="dwte"); _within(outs[0][1], pref, 1e-5, name="dwpe")
