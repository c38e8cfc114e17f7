"""GPT-J on the fp32 rollout engine — the second model family of the reference (`llm_rl_scripts/wordle/{bc,ilql,mc,ppo,online_filtered_bc}/train_*.py`
run GPT-J; `LLM_RL/algorithms/*/gptj/` mirrors every GPT-2 interface).  Inference only, in the reference's default float32 arithmetic.

What differs from GPT-2 (`gpt2_f32_engine.GPT2EngineF32`):
  * no learned position table: q and k are rotated by GPT-J's interleaved rotary embedding on the first `rotary_dim` dims of each head
    (`lmrl_rope_gptj_f32_async`, csrc/attn_rope_f32.hip) with the positions `lmrl_chunk_begin_f32` produces; the K cache stores the ROTATED k;
  * head dim 64, 128 or 256 (`lmrl_attn_cached_hd_f32`; GPT-J-6B: 16 heads of 256);
  * one LayerNorm per block feeds attention and MLP in parallel: x = x + out_proj(attn(ln_1(x))) + fc_out(gelu_new(fc_in(ln_1(x))));
  * q / k / v / out projections carry no bias; the LM head is untied and has a bias.

Every product is `lmrl_sgemm` (the f32-input MFMA, bit-for-bit an fmaf chain); LayerNorm / gelu / the sampler are the kernels the GPT-2 fp32 engine
uses.  `KVSessionGPTJ` has the interface of `KVSessionF32` that the text policies use, so `policies.GPT2PPOPolicy` (`GPTJPPOPolicy`),
`interact_environment` and `text_env_eval` drive it unchanged.  Not implemented for GPT-J, and refused with `GPTJUnsupported`: the train steps, the
bf16 engine, the device-resident rollout loops, the ILQL / MC value policies and beam search.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import _lib
from .gpt2 import SampleParams
from .train import ops

HEAD_DIMS = (64, 128, 256)


class GPTJUnsupported(NotImplementedError):
    pass


@dataclass
class GPTJConfig:
    n_layer: int = 28
    n_head: int = 16
    d_model: int = 4096
    rotary_dim: Optional[int] = 64      # None: the whole head
    d_ff: Optional[int] = None          # None: 4 * d_model
    vocab: int = 50400
    n_pos: int = 2048
    ln_eps: float = 1e-5
    initializer_range: float = 0.02

    model_family = "gptj"

    def __post_init__(self):
        if self.d_ff is None:
            self.d_ff = 4 * self.d_model
        if self.d_model % self.n_head:
            raise ValueError(f"d_model = {self.d_model} is not a multiple of n_head = {self.n_head}")
        if self.rotary_dim is None:
            self.rotary_dim = self.head_dim
        if self.rotary_dim <= 0 or self.rotary_dim % 2 or self.rotary_dim > self.head_dim:
            raise ValueError(f"rotary_dim = {self.rotary_dim} must be even and within the head dim {self.head_dim}")

    @property
    def head_dim(self) -> int:
        return self.d_model // self.n_head

    @property
    def vocab_padded(self) -> int:
        return (self.vocab + 127) // 128 * 128

    @classmethod
    def gptj_6b(cls) -> "GPTJConfig":
        return cls(28, 16, 4096, 64, 16384, 50400, 2048)

    @classmethod
    def from_hf(cls, cfg_json: dict) -> "GPTJConfig":
        """From the fields of an HF `GPTJConfig` / its `config.json` (a dict, or any object with those attributes)."""
        get = cfg_json.get if isinstance(cfg_json, dict) else (lambda k, default=None: getattr(cfg_json, k, default))
        if get("model_type", "gptj") != "gptj":
            raise ValueError(f"not a GPT-J configuration: model_type = {get('model_type')!r}")
        if get("activation_function", "gelu_new") != "gelu_new":
            raise ValueError(f"GPT-J activation {get('activation_function')!r}: only gelu_new is implemented")
        d = int(get("n_embd", 4096))
        return cls(n_layer=int(get("n_layer", 28)), n_head=int(get("n_head", 16)), d_model=d,
                   rotary_dim=None if get("rotary_dim", 64) is None else int(get("rotary_dim", 64)),
                   d_ff=int(get("n_inner") or 4 * d), vocab=int(get("vocab_size", 50400)), n_pos=int(get("n_positions", 2048)),
                   ln_eps=float(get("layer_norm_epsilon", 1e-5)), initializer_range=float(get("initializer_range", 0.02)))

    def to_hf(self) -> dict:
        return dict(model_type="gptj", n_layer=self.n_layer, n_head=self.n_head, n_embd=self.d_model, rotary_dim=self.rotary_dim, n_inner=self.d_ff,
                    vocab_size=self.vocab, n_positions=self.n_pos, layer_norm_epsilon=self.ln_eps, activation_function="gelu_new",
                    initializer_range=self.initializer_range, tie_word_embeddings=False)


def is_gptj(obj) -> bool:
    """A GPT-J engine, configuration, or anything that carries one as `cfg` / `engine`."""
    for o in (obj, getattr(obj, "cfg", None), getattr(obj, "engine", None), getattr(getattr(obj, "engine", None), "cfg", None)):
        if getattr(o, "model_family", None) == "gptj":
            return True
    return False


def refuse_gptj(what: str, *objs) -> None:
    """Raise `GPTJUnsupported` if any of `objs` is a GPT-J engine / model.  Host logic only: nothing here touches the GPU."""
    if any(o is not None and is_gptj(o) for o in objs):
        raise GPTJUnsupported(f"{what} is not implemented for GPT-J: a GPTJEngineF32 serves fp32 inference only — KV sessions, the text policies "
                              "(GPTJPPOPolicy, sampling or greedy), interact_environment / text_env_eval and harness bc-eval / maze-eval.  GPT-J "
                              "training, the bf16 engine, the device-resident rollout loops, the ILQL / MC value policies and beam search are not "
                              "implemented; use a GPT-2 engine there")


def rotary_sincos_table(n_pos: int, rotary_dim: int):
    """fp32 [n_pos][rotary_dim] = [sin | cos] of pos * 10000^(-2i / rotary_dim), i < rotary_dim / 2 — HF's `create_sinusoidal_positions`
    operation for operation (int64 arange / dim -> float32, 10000 ** that, reciprocal, outer product with float32 positions, sin and cos in
    float32), so the table is that function's bit for bit."""
    import torch
    inv_freq = 1.0 / (10000 ** (torch.arange(0, rotary_dim, 2, dtype=torch.int64) / rotary_dim))
    angle = torch.einsum("i , j -> i j", torch.arange(n_pos, dtype=torch.int64).float(), inv_freq).float()
    return torch.cat((torch.sin(angle), torch.cos(angle)), dim=1)


def init_hf_style_gptj_state_dict(cfg: GPTJConfig, seed: int = 0) -> Dict[str, "torch.Tensor"]:
    """Random-init weights with HF PyTorch GPT-J names and shapes (`nn.Linear` weights are [out][in]; normal(0, initializer_range); LN = 1 / 0;
    biases zero — HF's `_init_weights`)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    n = lambda *shape: torch.randn(*shape, generator=g) * cfg.initializer_range
    d = cfg.d_model
    sd = {"transformer.wte.weight": n(cfg.vocab, d), "transformer.ln_f.weight": torch.ones(d), "transformer.ln_f.bias": torch.zeros(d),
          "lm_head.weight": n(cfg.vocab, d), "lm_head.bias": torch.zeros(cfg.vocab)}
    for l in range(cfg.n_layer):
        p = f"transformer.h.{l}."
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = torch.ones(d), torch.zeros(d)
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"attn.{name}.weight"] = n(d, d)
        sd[p + "mlp.fc_in.weight"], sd[p + "mlp.fc_in.bias"] = n(cfg.d_ff, d), torch.zeros(cfg.d_ff)
        sd[p + "mlp.fc_out.weight"], sd[p + "mlp.fc_out.bias"] = n(d, cfg.d_ff), torch.zeros(d)
    return sd


def fuse_qkv(wq, wk, wv):
    """Three HF `nn.Linear` weights [out][in] -> the engine's one operand [in][3 out] = [Wq^T | Wk^T | Wv^T] (h . W gives the [q | k | v] row)."""
    import torch
    return torch.cat([wq.t(), wk.t(), wv.t()], dim=1).contiguous()


def split_qkv(w):
    """Inverse of `fuse_qkv`: [in][3 out] -> (wq, wk, wv), each [out][in]."""
    d = w.shape[1] // 3
    return tuple(w[:, i * d:(i + 1) * d].t().contiguous() for i in range(3))


def _strip(sd):
    return {(k[len("transformer."):] if k.startswith("transformer.") else k): v for k, v in sd.items()}


class GPTJEngineF32:
    model_family = "gptj"
    matmul = "f32"

    def __init__(self, cfg: GPTJConfig, state_dict: Dict[str, "torch.Tensor"], device=None, matmul: str = "f32"):
        import torch
        if matmul != "f32":
            raise ValueError(f"GPTJEngineF32 supports matmul = 'f32' only (every product on the f32-input MFMA), not {matmul!r}")
        if cfg.head_dim not in HEAD_DIMS:
            raise ValueError(f"GPT-J head dim {cfg.head_dim}: the attention kernel is built for {HEAD_DIMS}")
        self.cfg = cfg
        self.device = device or _lib.require_gpu()
        self._L = _lib.lib()
        sd = _strip(state_dict)
        as_t = lambda v: v if hasattr(v, "to") else torch.from_numpy(np.asarray(v))
        f32 = lambda t: as_t(t).to(self.device, torch.float32).contiguous()
        d, V, Vp = cfg.d_model, cfg.vocab, cfg.vocab_padded
        self.wte = torch.zeros(Vp, d, dtype=torch.float32, device=self.device)
        self.wte[:V] = f32(sd["wte.weight"])[:V]
        self.lnf_g, self.lnf_b = f32(sd["ln_f.weight"]), f32(sd["ln_f.bias"])
        # untied LM head [vocab_padded][d] + bias; rows past the vocabulary are zero (their logits are 0 and the sampler never reads them)
        self.lm_w = torch.zeros(Vp, d, dtype=torch.float32, device=self.device)
        self.lm_w[:V] = f32(sd["lm_head.weight"])[:V]
        self.lm_b = torch.zeros(Vp, dtype=torch.float32, device=self.device)
        self.lm_b[:V] = f32(sd["lm_head.bias"])[:V]
        self.layers = []
        for l in range(cfg.n_layer):
            p = f"h.{l}."
            self.layers.append({
                "ln_g": f32(sd[p + "ln_1.weight"]), "ln_b": f32(sd[p + "ln_1.bias"]),
                "wqkv": f32(fuse_qkv(*(as_t(sd[p + f"attn.{n}_proj.weight"]) for n in "qkv"))),           # [d][3 d], no bias
                "wout": f32(as_t(sd[p + "attn.out_proj.weight"]).t()),                                    # [d][d], no bias
                "w_in": f32(as_t(sd[p + "mlp.fc_in.weight"]).t()), "b_in": f32(sd[p + "mlp.fc_in.bias"]),   # [d][d_ff]
                "w_out": f32(as_t(sd[p + "mlp.fc_out.weight"]).t()), "b_out": f32(sd[p + "mlp.fc_out.bias"]),  # [d_ff][d]
            })
        self.sincos = rotary_sincos_table(cfg.n_pos, cfg.rotary_dim).to(self.device).contiguous()
        self._no_wpe = torch.zeros(1, d, dtype=torch.float32, device=self.device)       # lmrl_embed_fwd adds a position row: GPT-J has none

    def splitk_ws_bytes(self, rows: int) -> int:
        """Bytes of split-K partial-sum workspace ONE caller needs for this engine's products on `rows` rows (as `GPT2EngineF32.splitk_ws_bytes`: the
        workspace belongs to the caller — a KV session sizes it once, before any graph capture)."""
        c, need = self.cfg, 0
        for k, n in ((c.d_model, 3 * c.d_model), (c.d_model, c.d_model), (c.d_model, c.d_ff), (c.d_ff, c.d_model)):
            need = max(need, int(self._L.lmrl_sgemm_ws_bytes(rows, n, k, 1)))
        return need

    def lm_head_ws_bytes(self, rows: int) -> int:
        return int(self._L.lmrl_sgemm_ws_bytes(rows, self.cfg.vocab_padded, self.cfg.d_model, 1))

    @classmethod
    def random_init(cls, cfg: GPTJConfig, seed: int = 0, device=None, matmul: str = "f32") -> "GPTJEngineF32":
        return cls(cfg, init_hf_style_gptj_state_dict(cfg, seed), device, matmul=matmul)

    def session(self, batch: int, tmax: int, flags: int = 0) -> "KVSessionGPTJ":
        return KVSessionGPTJ(self, batch, tmax)

    def check_value_head(self, head: dict) -> None:
        refuse_gptj("A value head (the ILQL / MC value policies)", self)


class KVSessionGPTJ:
    """`KVSessionF32` for GPT-J: persistent fp32 K/V cache [layer][K|V][B][tmax][d] (K rows rotated) + workspaces per chunk size."""

    def __init__(self, eng: GPTJEngineF32, batch: int, tmax: int):
        import torch
        t = torch
        self.eng, self.B, self.tmax, self.flags = eng, batch, tmax, 0
        c, dev = eng.cfg, eng.device
        self.kv = t.zeros(c.n_layer, 2, batch, tmax, c.d_model, dtype=t.float32, device=dev)
        self.len = t.zeros(batch, dtype=t.int32, device=dev)
        self.last_hidden = t.zeros(batch, c.d_model, dtype=t.float32, device=dev)      # ln_f of each env's last token
        self._last_x = t.zeros(batch, c.d_model, dtype=t.float32, device=dev)
        self.token = t.zeros(batch, dtype=t.int32, device=dev)
        self.logprob = t.zeros(batch, dtype=t.float32, device=dev)
        self.logits = t.zeros(batch, c.vocab_padded, dtype=t.float32, device=dev)
        nlm = eng.lm_head_ws_bytes(batch)          # the LM head's split-K workspace: this session's, sized once
        self._lm_ws = t.empty(nlm, dtype=t.uint8, device=dev) if nlm else None
        self._ws = {}
        self._len_bound = 0

    def _bufs(self, C):
        import torch
        t = torch
        if C not in self._ws:
            c, R, dev = self.eng.cfg, self.B * C, self.eng.device
            nsk = self.eng.splitk_ws_bytes(R)
            f = lambda *s: t.empty(*s, dtype=t.float32, device=dev)
            self._ws[C] = dict(ids=t.zeros(R, dtype=t.int32, device=dev), pos=t.zeros(R, dtype=t.int32, device=dev),
                               pos0=t.zeros(R, dtype=t.int32, device=dev),        # row of the (empty) position table for lmrl_embed_fwd: always 0
                               x=f(R, c.d_model), h=f(R, c.d_model), r=f(R, c.d_model), r2=f(R, c.d_model), qkv=f(R, 3 * c.d_model),
                               att=f(R, c.d_model), ff=f(R, c.d_ff), mean=f(R), rstd=f(R),
                               # split-K partial sums of THIS session's products: per session and per chunk size, sized once (captured graphs hold
                               # the pointer; lanes on other streams own theirs)
                               splitk=t.empty(nsk, dtype=t.uint8, device=dev) if nsk else None)
        return self._ws[C]

    def reset(self):
        self.len.zero_()
        self._len_bound = 0

    def forward(self, tokens, cnt, chunk: int, all_hidden=None, len_bound_after: Optional[int] = None):
        """tokens int32 [B*chunk], cnt int32 [B] (env b's new tokens are slots b*chunk .. b*chunk + cnt[b] - 1): appends them to the cache,
        advances self.len, leaves ln_f(hidden of each env's last new token) in self.last_hidden; `all_hidden` fp32 [B*chunk][d] gets ln_f of every
        row.  No host synchronisation and, after the first call at a chunk size, no allocation: capturable in a hipGraph."""
        e, c, L, sp = self.eng, self.eng.cfg, self.eng._L, _lib.stream_ptr()
        C, B, d, R = chunk, self.B, c.d_model, self.B * chunk
        bound = self._len_bound + C if len_bound_after is None else int(len_bound_after)
        if bound > self.tmax:
            raise _lib.LmrlError(f"KV cache overflow: up to {bound} positions into a cache of tmax = {self.tmax}")
        if bound > c.n_pos:      # the host-side bound on every position handed to the rotary kernel (its table has n_pos rows)
            raise _lib.LmrlError(f"up to {bound} positions, the model's rotary table holds n_pos = {c.n_pos}")
        self._len_bound = bound
        w = self._bufs(C)
        w["ids"].copy_(tokens.view(-1)[:R])
        _lib.check(L.lmrl_chunk_begin_f32(_lib.ptr(self.len), _lib.ptr(cnt), _lib.ptr(w["ids"]), _lib.ptr(w["pos"]), B, C, c.n_pos, sp), "lmrl_chunk_begin_f32")
        x, h, r, r2, qkv, att, ff, sk = w["x"], w["h"], w["r"], w["r2"], w["qkv"], w["att"], w["ff"], w["splitk"]
        ops.embed_fwd(e.wte, e._no_wpe, w["ids"], w["pos0"], x, R, d, vocab=c.vocab_padded)     # x = wte[id] (+ the zero row); dead slots carry id 0
        pending = None                                   # the block's a + m, added to x inside the next LayerNorm launch (lmrl_layernorm_add_fwd)
        for l, p in enumerate(e.layers):
            ops.layernorm_add_fwd(x, pending, p["ln_g"], p["ln_b"], h, w["mean"], w["rstd"], None, 0, R, d, c.ln_eps)
            ops.sgemm(h, p["wqkv"], qkv, R, 3 * d, d, lda=d, ldb=3 * d, ldc=3 * d, ws=sk)
            _lib.check(L.lmrl_rope_gptj_f32_async(_lib.ptr(qkv), _lib.ptr(w["pos"]), _lib.ptr(e.sincos), R, c.n_head, c.head_dim, c.rotary_dim, c.n_pos, sp),
                       "lmrl_rope_gptj_f32_async")
            _lib.check(L.lmrl_attn_cached_hd_f32(_lib.ptr(qkv), _lib.ptr(self.kv[l, 0]), _lib.ptr(self.kv[l, 1]), _lib.ptr(self.len), _lib.ptr(cnt),
                                                 _lib.ptr(att), B, C, c.n_head, c.head_dim, self.tmax, sp), "lmrl_attn_cached_hd_f32")
            ops.sgemm(att, p["wout"], r, R, d, d, lda=d, ldb=d, ldc=d, ws=sk)                              # a = att . Wout
            ops.sgemm(h, p["w_in"], ff, R, c.d_ff, d, lda=d, ldb=c.d_ff, ldc=c.d_ff, bias=p["b_in"], ws=sk)
            ops.gelu_fwd(ff, ff)
            ops.sgemm(ff, p["w_out"], r2, R, d, c.d_ff, lda=c.d_ff, ldb=d, ldc=d, bias=p["b_out"], ws=sk)  # m = fc_out(gelu_new(fc_in(h)))
            ops.axpby(1.0, r, 1.0, r2, r)                                                                  # a + m
            pending = r
        if all_hidden is not None:
            ops.layernorm_add_fwd(x, pending, e.lnf_g, e.lnf_b, all_hidden, w["mean"], w["rstd"], None, 0, R, d, c.ln_eps)
        elif pending is not None:
            ops.axpby(1.0, pending, 1.0, x, x)
        _lib.check(L.lmrl_chunk_end_f32(_lib.ptr(x), _lib.ptr(cnt), _lib.ptr(self._last_x), _lib.ptr(self.len), B, C, d, sp), "lmrl_chunk_end_f32")
        ops.layernorm_fwd(self._last_x, e.lnf_g, e.lnf_b, self.last_hidden, w["mean"], w["rstd"], B, d, c.ln_eps)
        return self.last_hidden

    def set_len(self, lens):
        """Truncate / set every env's cache length from the host (int array [B]), as `KVSessionF32.set_len`."""
        import torch
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        assert lens.shape == (self.B,) and int(lens.max(initial=0)) <= self.tmax
        self.len.copy_(torch.from_numpy(lens))
        self._len_bound = int(lens.max(initial=0))

    def broadcast_prefix_from(self, src: "KVSessionGPTJ", n_pos: int):
        """Every env starts with the n_pos-token prefix held by the 1-env session `src` (device-to-device row copies)."""
        assert src.B == 1 and src.eng is self.eng
        self.kv[:, :, :, :n_pos].copy_(src.kv[:, :, :, :n_pos].expand(-1, -1, self.B, -1, -1))
        self._last_x.copy_(src._last_x.expand(self.B, -1))
        self.last_hidden.copy_(src.last_hidden.expand(self.B, -1))
        self.len.fill_(n_pos)
        self._len_bound = max(self._len_bound, n_pos)

    def lm_logits(self, hidden=None):
        """logits fp32 [B][vocab_padded] = hidden . lm_head^T + lm_head.bias (untied head; padded rows are zero) into self.logits."""
        c, e = self.eng.cfg, self.eng
        h = self.last_hidden if hidden is None else hidden
        ops.sgemm(h, e.lm_w, self.logits, self.B, c.vocab_padded, c.d_model, trans_b=True, lda=c.d_model, ldb=c.d_model, ldc=c.vocab_padded,
                  bias=e.lm_b, ws=self._lm_ws)
        return self.logits

    def sample(self, params: SampleParams, steer_tok=None, active=None, hidden=None, logits_out=None, q1=None, q2=None, want_logprob: bool = True):
        """One token per env from `hidden` (default: last_hidden): the fp32 LM head into materialised logits, then `lmrl_sample_logits_steer` — the
        sampler of `KVSessionF32` (same random streams, temperature, top-k and top-p)."""
        if q1 is not None or q2 is not None:
            refuse_gptj("Sampling with Q heads (the ILQL / MC value policies)", self.eng)
        c = self.eng.cfg
        lg = self.lm_logits(hidden)
        _lib.check(self.eng._L.lmrl_sample_logits_steer(_lib.ptr(lg), c.vocab_padded, self.B, c.vocab, ctypes.byref(params), _lib.ptr(steer_tok),
                                                        _lib.ptr(active), _lib.ptr(self.token), _lib.ptr(self.logprob) if want_logprob else None,
                                                        _lib.stream_ptr()), "lmrl_sample_logits_steer")
        if logits_out is not None:
            logits_out.copy_(lg)
        return self.token, (self.logprob if want_logprob else None)
