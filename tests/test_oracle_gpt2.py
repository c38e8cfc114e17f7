"""Pins oracle/gpt2.py against the installed HF PyTorch GPT-2 (CPU)."""
import pytest
import torch


def test_oracle_gpt2_matches_hf_pytorch():
    transformers = pytest.importorskip("transformers")
    from oracle import gpt2 as O
    cfg = transformers.GPT2Config(vocab_size=211, n_positions=48, n_embd=64, n_layer=3, n_head=4,
                                  resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
    torch.manual_seed(0)
    model = transformers.GPT2LMHeadModel(cfg).eval()
    # give LN params / biases non-trivial values
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    sd = {k[len("transformer."):]: v for k, v in model.state_dict().items() if k.startswith("transformer.") and not k.endswith(".attn.bias") and "masked_bias" not in k}
    ids = torch.randint(0, 211, (3, 17))
    with torch.no_grad():
        ref = model(ids).logits
    got = O.forward(sd, ids, n_head=4, dtype=torch.float32)
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)
    # padded batch with attention mask + explicit positions (how initialize_attn_mask_pos_ids feeds the model)
    am = torch.ones(3, 17, dtype=torch.long); am[1, 12:] = 0; am[2, 5:] = 0
    pos = (am.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        ref = model(ids, attention_mask=am, position_ids=pos).logits
    got = O.forward(sd, ids, n_head=4, attention_mask=am, position_ids=pos, dtype=torch.float32)
    m = am.bool()
    torch.testing.assert_close(got[m], ref[m], rtol=1e-4, atol=1e-4)


def _hf_layer_kv(pkv, l):
    """(K, V) of layer l from HF `past_key_values` [B, H, T, hd], across the cache classes of transformers releases."""
    if hasattr(pkv, "layers"):
        return pkv.layers[l].keys, pkv.layers[l].values
    if hasattr(pkv, "key_cache"):
        return pkv.key_cache[l], pkv.value_cache[l]
    return pkv[l][0], pkv[l][1]


@pytest.mark.parametrize("masked", [False, True])
def test_oracle_gpt2_kv_matches_hf_past_key_values(masked):
    """`forward(..., return_kv=True)`: every layer's K and V [B, T, d] (heads interleaved as in c_attn's columns, the engine's cache
    layout) equal HF's `past_key_values` (use_cache=True), and the logits / hidden states are the same as without the flag."""
    transformers = pytest.importorskip("transformers")
    from oracle import gpt2 as O
    n_layer, n_head, d = 3, 4, 64
    cfg = transformers.GPT2Config(vocab_size=211, n_positions=48, n_embd=d, n_layer=n_layer, n_head=n_head,
                                  resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
    torch.manual_seed(1)
    model = transformers.GPT2LMHeadModel(cfg).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    sd = {k[len("transformer."):]: v for k, v in model.state_dict().items() if k.startswith("transformer.") and not k.endswith(".attn.bias") and "masked_bias" not in k}
    B, T = 3, 23
    ids = torch.randint(0, 211, (B, T))
    kw, hw = {}, {}
    if masked:
        am = torch.ones(B, T, dtype=torch.long); am[1, 15:] = 0; am[2, 6:] = 0
        pos = (am.cumsum(-1) - 1).clamp(min=0)
        kw = dict(attention_mask=am, position_ids=pos)
        hw = dict(attention_mask=am, position_ids=pos)
    with torch.no_grad():
        out = model(ids, use_cache=True, **hw)
    logits, hid, (ks, vs) = O.forward(sd, ids, n_head=n_head, dtype=torch.float32, return_hidden=True, return_kv=True, **kw)
    logits0, hid0 = O.forward(sd, ids, n_head=n_head, dtype=torch.float32, return_hidden=True, **kw)
    assert torch.equal(logits, logits0) and torch.equal(hid, hid0)
    assert len(ks) == len(vs) == n_layer
    for l in range(n_layer):
        hk, hv = _hf_layer_kv(out.past_key_values, l)
        assert ks[l].shape == vs[l].shape == (B, T, d)
        # [B, H, T, hd] -> [B, T, H * hd]: head h at columns [h * hd, (h + 1) * hd)
        torch.testing.assert_close(ks[l], hk.transpose(1, 2).reshape(B, T, d), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(vs[l], hv.transpose(1, 2).reshape(B, T, d), rtol=1e-5, atol=1e-5)
    # float64: the same rows as float32 to float32 rounding (the GPU tier compares against the float64 form)
    _, (k64, v64) = O.forward(sd, ids, n_head=n_head, dtype=torch.float64, return_kv=True, **kw)
    assert k64[0].dtype == torch.float64
    for l in range(n_layer):
        torch.testing.assert_close(k64[l].float(), ks[l], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(v64[l].float(), vs[l], rtol=1e-5, atol=1e-5)


def test_philox_known_answer():
    # Random123 known-answer test vector for philox4x32-10: counter = key = 0 and all-ones
    import numpy as np
    from oracle.gpt2 import philox4x32_10
    o = philox4x32_10([0], [0], [0], [0], 0, 0)
    assert [int(x[0]) for x in o] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    o = philox4x32_10([0xffffffff], [0xffffffff], [0xffffffff], [0xffffffff], 0xffffffff, 0xffffffff)
    assert [int(x[0]) for x in o] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_gumbel_noise_is_finite_for_extreme_bits():
    # u must stay strictly inside (0, 1) for every 32-bit draw (fp32 rounding of the +0.5 offset)
    import numpy as np
    for bits in (0, 1, 0xFFFFFFFF, 0xFFFFFE00, 0x80000000):
        u = (np.float32(bits >> 9) + np.float32(0.5)) * np.float32(1.1920928955078125e-07)
        assert 0.0 < float(u) < 1.0
        assert np.isfinite(-np.log(-np.log(u)))
