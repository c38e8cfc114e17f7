"""CPU tier of the GPT-J fp32 engine (`lmrl_gym_amd.gptj_f32_engine`): everything that needs no GPU — the rotary table against HF's own function
bit for bit, the q/k/v fusion and the flax-name translation as exact round trips, configuration parsing, the state-dict names against the installed
`transformers` GPT-J, the refusals of every path GPT-J does not run on, the compat import path and the C ABI surface of the new symbols."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401  (shim -> lmrl-gym_amd/)
from conftest import ROOT

torch = pytest.importorskip("torch")

NEW_SYMBOLS = ("lmrl_rope_gptj_f32", "lmrl_rope_gptj_f32_async", "lmrl_attn_cached_hd_f32", "lmrl_attn_hd_key_tile")


def _tiny_cfg(**kw):
    from lmrl_gym_amd.gptj_f32_engine import GPTJConfig
    return GPTJConfig(**{**dict(n_layer=2, n_head=2, d_model=128, rotary_dim=16, vocab=96, n_pos=64), **kw})


@pytest.mark.parametrize("rotary_dim", [16, 64])
def test_rotary_table_equals_hf_create_sinusoidal_positions_bit_for_bit(rotary_dim):
    from transformers.models.gptj.modeling_gptj import create_sinusoidal_positions
    from lmrl_gym_amd.gptj_f32_engine import rotary_sincos_table
    ours, ref = rotary_sincos_table(64, rotary_dim), create_sinusoidal_positions(64, rotary_dim)
    assert ours.dtype == torch.float32 and tuple(ours.shape) == (64, rotary_dim) == tuple(ref.shape)
    assert np.array_equal(ours.numpy().view(np.uint32), ref.float().numpy().view(np.uint32))
    # layout [sin | cos]: position 0 is the identity rotation, and the first pair's angle is the position itself
    assert np.all(ours[0, : rotary_dim // 2].numpy() == 0) and np.all(ours[0, rotary_dim // 2:].numpy() == 1)
    assert ours[3, 0].item() == np.sin(np.float32(3)) and ours[3, rotary_dim // 2].item() == np.cos(np.float32(3))


def test_state_dict_names_and_shapes_are_those_of_hf_pytorch_gptj():
    from transformers import GPTJConfig as HFConfig, GPTJForCausalLM
    from lmrl_gym_amd.gptj_f32_engine import GPTJConfig, init_hf_style_gptj_state_dict
    cfg = _tiny_cfg()
    sd = init_hf_style_gptj_state_dict(cfg, seed=1)
    hf = GPTJForCausalLM(HFConfig(**cfg.to_hf()))
    ref = {k: tuple(v.shape) for k, v in hf.state_dict().items() if not k.endswith(("attn.bias", "attn.masked_bias", "embed_positions"))}
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert "transformer.h.1.attn.q_proj.weight" in sd and "transformer.h.0.attn.q_proj.bias" not in sd and "lm_head.bias" in sd
    hf.load_state_dict(sd, strict=False)                 # the oracle of the GPU tier accepts these tensors
    again = GPTJConfig.from_hf(hf.config)
    assert again == cfg


def test_config_parsing():
    from lmrl_gym_amd.gptj_f32_engine import GPTJConfig
    c = GPTJConfig.from_hf(dict(model_type="gptj", n_layer=3, n_head=4, n_embd=512, rotary_dim=32, n_inner=None, vocab_size=1000, n_positions=256,
                                layer_norm_epsilon=1e-6))
    assert (c.n_layer, c.n_head, c.d_model, c.rotary_dim, c.d_ff, c.vocab, c.n_pos, c.ln_eps) == (3, 4, 512, 32, 2048, 1000, 256, 1e-6)
    assert c.head_dim == 128 and c.vocab_padded == 1024 and c.model_family == "gptj"
    assert GPTJConfig(2, 2, 256, None).rotary_dim == 128                       # None: the whole head
    assert GPTJConfig.from_hf(dict(n_layer=1, n_head=2, n_embd=128, rotary_dim=None)).rotary_dim == 64
    six = GPTJConfig.gptj_6b()
    assert (six.head_dim, six.rotary_dim, six.d_ff, six.vocab_padded) == (256, 64, 16384, 50432)
    assert GPTJConfig.from_hf(six.to_hf()) == six
    for bad in (dict(n_head=3, d_model=128), dict(rotary_dim=15), dict(rotary_dim=130)):
        with pytest.raises(ValueError):
            _tiny_cfg(**bad)
    with pytest.raises(ValueError):
        GPTJConfig.from_hf(dict(model_type="gpt2"))
    with pytest.raises(ValueError):
        GPTJConfig.from_hf(dict(activation_function="relu"))


def test_qkv_fusion_round_trips_exactly():
    from lmrl_gym_amd.gptj_f32_engine import fuse_qkv, split_qkv
    g = torch.Generator().manual_seed(0)
    wq, wk, wv = (torch.randn(48, 48, generator=g) for _ in range(3))
    w = fuse_qkv(wq, wk, wv)
    assert tuple(w.shape) == (48, 144) and w.is_contiguous()
    h = torch.randn(5, 48, generator=g).double()
    assert torch.equal(h @ w.double(), torch.cat([h @ wq.double().t(), h @ wk.double().t(), h @ wv.double().t()], dim=1))
    for a, b in zip(split_qkv(w), (wq, wk, wv)):
        assert torch.equal(a, b)


def test_flax_name_translation_and_checkpoint_directories_round_trip_exactly(tmp_path):
    from lmrl_gym_amd import checkpoints as C
    from lmrl_gym_amd.gptj_f32_engine import init_hf_style_gptj_state_dict
    cfg = _tiny_cfg()
    g = torch.Generator().manual_seed(2)
    sd = {k: (v + 0.1 * torch.randn(v.shape, generator=g)).numpy() for k, v in init_hf_style_gptj_state_dict(cfg, seed=1).items()}
    tree = C.state_dict_to_flax_gptj_params(sd)
    blk = tree["transformer"]["h"]["1"]
    assert set(tree) == {"transformer", "lm_head"} and set(tree["transformer"]) == {"wte", "h", "ln_f"} and set(blk) == {"ln_1", "attn", "mlp"}
    assert set(blk["attn"]) == {"q_proj", "k_proj", "v_proj", "out_proj"} and set(blk["attn"]["q_proj"]) == {"kernel"}
    assert blk["mlp"]["fc_in"]["kernel"].shape == (cfg.d_model, cfg.d_ff) and tree["lm_head"]["kernel"].shape == (cfg.d_model, cfg.vocab)   # [in][out]
    assert np.array_equal(blk["attn"]["q_proj"]["kernel"], sd["transformer.h.1.attn.q_proj.weight"].T)
    back = C.flax_gptj_params_to_state_dict(tree)
    assert set(back) == set(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)
    # the reference's directory layout (flax names) ...
    C.save_gptj_checkpoint(str(tmp_path / "flax"), cfg, sd)
    assert C.checkpoint_model_family(str(tmp_path / "flax")) == "gptj"
    cfg2, sd2 = C.load_gptj_checkpoint(str(tmp_path / "flax"))
    assert cfg2 == cfg and set(sd2) == set(sd) and all(np.array_equal(sd2[k], sd[k]) for k in sd)
    # ... and the HF PyTorch layout
    import json
    hfdir = tmp_path / "hf"
    hfdir.mkdir()
    (hfdir / "config.json").write_text(json.dumps(cfg.to_hf()))
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, str(hfdir / "pytorch_model.bin"))
    cfg3, sd3 = C.load_hf_pytorch_gptj(str(hfdir))
    assert cfg3 == cfg and set(sd3) == set(sd) and all(np.array_equal(sd3[k], sd[k]) for k in sd)
    with pytest.raises(ValueError):
        C._gptj_config({"rotary_dim": 16}, sd, "x")          # no n_head: refuse instead of guessing


def _stand_in_engine():
    """A GPT-J engine object without a GPU: the refusals look at the engine's family only."""
    from lmrl_gym_amd.gptj_f32_engine import GPTJEngineF32
    eng = GPTJEngineF32.__new__(GPTJEngineF32)
    eng.cfg = _tiny_cfg()
    return eng


class _Tok:
    pad_token_id, eos_token_id = 0, 1

    def encode(self, s):
        return [2 + (ord(c) % 90) for c in s]

    def decode(self, ids, **kw):
        return "".join(chr(32 + i) for i in ids)


def test_paths_out_of_scope_refuse_a_gptj_engine_without_touching_the_gpu(monkeypatch):
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.gptj_f32_engine import GPTJEngineF32, GPTJUnsupported
    from lmrl_gym_amd.algorithms.bc import GPT2BCTrain
    from lmrl_gym_amd.algorithms.ilql import GPT2ILQLTrain
    from lmrl_gym_amd.algorithms.mc_returns import GPT2MCTrain
    from lmrl_gym_amd.algorithms.ppo import GPT2PPOTrain
    from lmrl_gym_amd.chess_rollout import ChessRolloutEngine
    from lmrl_gym_amd.maze_rollout import MazeRolloutEngine
    from lmrl_gym_amd.policies import GPT2PPOPolicy, GPT2ValuePolicy, GPTJPPOPolicy
    from lmrl_gym_amd.rollout import WordleRolloutEngine
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine

    def no_gpu(*a, **k):
        raise AssertionError("a refusal touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "lib", no_gpu)
    eng, tok = _stand_in_engine(), _Tok()
    cases = {
        "WordleRolloutEngine": lambda: WordleRolloutEngine(eng, None, 4),
        "WordleRolloutEngine (value engine)": lambda: WordleRolloutEngine(object(), None, 4, value_engine=eng),
        "MazeRolloutEngine": lambda: MazeRolloutEngine(eng, tok, None, 4),
        "ChessRolloutEngine": lambda: ChessRolloutEngine(eng, tok, None, 4),
        "TwentyQuestionsRolloutEngine": lambda: TwentyQuestionsRolloutEngine(eng, eng, tok, None, 4, 8, 1, 64, 64),
        "TwentyQuestionsRolloutEngine (oracle)": lambda: TwentyQuestionsRolloutEngine(object(), eng, tok, None, 4, 8, 1, 64, 64),
        "GPT2ValuePolicy": lambda: GPT2ValuePolicy(eng, eng, {}, None, 1.0, tok),
        "num_beams": lambda: GPT2PPOPolicy(eng, tok, do_sample=False, num_beams=2),
        "num_beams (GPTJPPOPolicy)": lambda: GPTJPPOPolicy(eng, tok, do_sample=False, num_beams=4),
        "GPT2PPOTrain": lambda: GPT2PPOTrain(eng, None, 0, {}),
        "GPT2ILQLTrain": lambda: GPT2ILQLTrain(eng, None, None, None, 0, {}),
        "GPT2MCTrain": lambda: GPT2MCTrain(eng, None, 0, {}),
        "GPT2BCTrain": lambda: GPT2BCTrain(eng, 0),
        "value head": lambda: eng.check_value_head({}),
    }
    for name, make in cases.items():
        with pytest.raises(GPTJUnsupported, match="not implemented for GPT-J"):
            make()
    assert issubclass(GPTJUnsupported, NotImplementedError)
    # the one matmul mode
    with pytest.raises(ValueError, match="'f32'"):
        GPTJEngineF32(_tiny_cfg(), {}, matmul="bf16x3")
    # what stays in scope constructs: the text policy (sampling or greedy), under either name
    assert GPTJPPOPolicy(eng, tok, do_sample=False).engine is eng and GPT2PPOPolicy(eng, tok, top_k=5, top_p=0.9).top_k == 5
    with pytest.raises(TypeError):
        GPTJPPOPolicy(object(), tok)


def _harness():
    spec = importlib.util.spec_from_file_location("_harness_under_test", os.path.join(ROOT, "scripts", "harness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_harness_model_family_flag_and_refusals(tmp_path):
    from lmrl_gym_amd import checkpoints as C
    from lmrl_gym_amd.gptj_f32_engine import init_hf_style_gptj_state_dict
    H = _harness()
    C.save_gptj_checkpoint(str(tmp_path / "policy"), _tiny_cfg(), init_hf_style_gptj_state_dict(_tiny_cfg(), seed=3))
    cfg, sd = H._model(str(tmp_path / "policy"), 50257, "gptj")                 # --model <dir>: the checkpoint's own configuration
    assert cfg == _tiny_cfg() and torch.equal(sd["lm_head.weight"], init_hf_style_gptj_state_dict(_tiny_cfg(), seed=3)["lm_head.weight"])
    for cmd in ("bc-eval", "maze-eval"):
        assert H.build_parser().parse_args([cmd]).model_family == "gpt2"
        assert H.build_parser().parse_args([cmd, "--model-family", "gptj", "--model", "random:gptj-tiny"]).model_family == "gptj"
    cfg, sd = H._model("random:gptj-tiny", 300, "gptj")
    assert cfg.model_family == "gptj" and cfg.vocab == 300 and cfg.head_dim in (64, 128, 256) and "lm_head.bias" in sd
    with pytest.raises(SystemExit, match="--device-rollouts"):
        H.main(["bc-eval", "--model", "random:gptj-tiny", "--model-family", "gptj", "--device-rollouts", "1"])
    for cmd in ("ppo", "ilql", "filtered-bc"):
        with pytest.raises(SystemExit, match="GPT-J training is not implemented"):
            H.main([cmd, "--model", "random:gptj-tiny", "--model-family", "gptj"])
    with pytest.raises(SystemExit, match="beam"):
        H.main(["bc-eval", "--model", "random:gptj-tiny", "--model-family", "gptj", "--policy-num-beams", "2"])
    with pytest.raises(SystemExit, match="--model-family gptj"):
        H._model("random:gptj-tiny", 300)                        # a GPT-J size under the GPT-2 family
    with pytest.raises(SystemExit, match="random:gptj-tiny"):
        H._model("random:small", 300, "gptj")


def test_compat_import_path():
    root = os.path.join(ROOT, "compat")
    sys.path.insert(0, root)
    try:
        from LLM_RL.algorithms.ppo.gptj.interface import GPTJPPOPolicy
        import LLM_RL.algorithms.ppo.gptj as pkg
        from lmrl_gym_amd import policies as P
        assert GPTJPPOPolicy is P.GPTJPPOPolicy and issubclass(GPTJPPOPolicy, P.GPT2PPOPolicy) and pkg.__name__.endswith("ppo.gptj")
    finally:
        sys.path.remove(root)
        for k in [k for k in sys.modules if k == "LLM_RL" or k.startswith("LLM_RL.")]:
            del sys.modules[k]


def test_new_symbols_exported_declared_and_bound():
    """exported (the dynamic symbol table of the built library) = declared (include/lmrl_amd.h) = bound (`_lib._SIGS`), argument counts included."""
    from lmrl_gym_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    hdr = open(os.path.join(ROOT, "include", "lmrl_amd.h")).read()
    src = open(os.path.join(ROOT, "lmrl-gym_amd", "csrc", "attn_rope_f32.hip")).read()
    defined_here = set(re.findall(r"^int (lmrl_[a-z0-9_]+)\(", src, flags=re.M))
    assert defined_here == set(NEW_SYMBOLS)                     # the file exports nothing the header does not declare
    for name in NEW_SYMBOLS:
        assert name in exported, f"{name} not exported"
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, flags=re.S)
        assert m, f"{name} not declared"
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert name in _lib._SIGS, f"{name} not bound"
        res, args = _lib._SIGS[name]
        assert res is _lib.c_int and len(args) == len(params), (name, len(args), len(params))
        if params:
            assert params[-1].strip() == "void *stream" and args[-1] is _lib.c_void_p
    assert _lib.lib().lmrl_attn_hd_key_tile() == 8
