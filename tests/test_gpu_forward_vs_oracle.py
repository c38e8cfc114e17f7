"""GPU tier: the rollout engine's forward (`lmrl_gpt2_forward`, csrc/gpt2.hip; the fp32 twin csrc/attn_cached_f32.hip) against the float64
oracle (oracle/gpt2.py, pinned to HF GPT-2 by tests/test_oracle_gpt2.py) PER LAYER, at full context (n_pos = tmax = 1024) and on every
kernel path that is not asserted bit-identical to the default one elsewhere.

One harness: a `KVSession` is driven through a schedule of chunk and decode forwards; afterwards every layer's K and V cache rows at every
live position of every checked env, `last_hidden` after every forward and `all_hidden` where a chunk forward returns it are compared with
ONE float64 oracle pass over each env's final token sequence (causal: position p of the oracle depends on tokens <= p only).  Layer l + 1's
K/V rows are a function of layer l's attention and MLP, so 2-layer models pin both layers' products and attention.  Metrics: relative
Frobenius error and the worst per-row max-abs error scaled by the row maximum (an error confined to a few rows or positions cannot hide
in the norm); the hidden states are also reported for the decode forwards' rows alone (`dec_*`), where a decode-only error concentrates.
Each variant session is also compared with the default session on the same tokens (`dkv_*`, `dhid_*`): two independent kernel paths
(the VALU attention kernels against the single-sweep decode / MFMA chunk kernels, the skinny products and the SPLIT = 4 decode attention
against the tiles and the one-wave decode, the stand-alone LayerNorm against the fold) agree far more closely than either agrees with
the float64 oracle, so a systematic error of a few percent on a fraction of the cached positions — below the oracle comparison's bf16
noise in the peaked regime — still fails that bound.  Variants that are not bit-identical to the default also satisfy err_variant <= 1.25 err_default + floor on the same inputs.

Weights: `plain` = init_hf_style_state_dict with non-trivial LN / bias values; `sharp` = two residual dimensions at magnitudes in the
hundreds (+144 / -112 through wpe columns, small LN gains on them, as trained GPT-2 checkpoints have: exercises the LN fold's mu * colsum
and its moment sums at scale), the Q / K columns of c_attn scaled so that layer 0's attention rows are peaked (asserted: median top-1
weight >= 0.5 over the checked queries) and c_proj of the attention scaled by 4, so that attention outputs carry most of a layer's
residual update.  With near-uniform attention a kernel that drops or mis-weights cached positions moves the
output by less than bf16 noise.

Cases and the kernel instantiations they reach (dense products: gemm_dispatch.h `gemm_launch_ln_nq<EPI, NQ>` for the LN-folded qkv / fc
(EPI_BF16_LN / EPI_GELU_BF16_LN, NQ = 1 / 3 / 4 / 5 at d = 128 / 768 / 1024 / 1280) and proj / fc2 of every layer but the last
(EPI_RESID_F32_STATS, NQ = 0); the last layer's fc2 is `gemm_launch<EPI_RESID_F32>`; skinny_gemm.h `skinny_launch<EPI>` with
STEPS = K / 256):

* test_long_context_d768 (B = 12, d = 768): decode steps from cache lengths starting at 0, 1, 7, 31, 95, 127, 255, 511, 1000 and 1016
  (up to 8 steps each: L0 covers 0, 1, 7, 8, 31..33, 95..97, 127..129, 255, 256, 511, 512, 1000, 1022, 1023) in one ragged batch (the
  env at 1016 writes position 1023 = the last slot of tmax = 1024), after a
  prefill of an 8-token chunk with ragged counts then 16-token chunks (`attention_chunk_mfma_kernel<16>`) over cached prefixes that are
  not multiples of 32, then a closing 8-token chunk (`attention_chunk_mfma_kernel<8>`; with all_hidden), cnt = 0 rows throughout, a
  decode step with finished rows between live ones and a decode step with every cnt = 0 (lengths, cache and last_hidden unchanged).
  Sessions on the same tokens:
    default        decode `attention_decode_kernel<4, false, false, 1>`; qkv / fc / proj `gemm_bf16_glds<64, 64, 4, *, 3>` (M = 12 and
                   M = 192 chunk rows), last-layer chunk rows `gemm_bf16_glds<64, 64, 4>`, fc2 `gemm8<64, 64, 4, 2, 4>` (K = 3072)
    skinny         FWD_SKINNY: decode products `skinny_gemm_kernel<*, 3 | 12, 1>`, decode attention `attention_decode_split_kernel<4, false>`
                   (SPLIT = 4: position batches strided by 128)
    skinny_ragged  FWD_SKINNY | FWD_RAGGED_ALWAYS: the same on compacted rows (m_dev)
    valu           FWD_ATTN_VALU: decode `attention_kernel<1>`, the 8-token chunks `attention_kernel<8>`
    ln_standalone  FWD_LN_STANDALONE: `layernorm_kernel<4>` + `gemm_launch<EPI_BF16 | EPI_GELU_BF16 | EPI_RESID_F32>`, `embed_ln_kernel<4>`
* test_long_context_width[128 | 1024 | 1280] (B = 4, cache lengths 0 / 129 / 600 / 1016 -> 1023): the same schedule at NQ = 1 / 4 / 5
  (`gemm_bf16_glds<64, 64, 4, EPI_BF16_LN | EPI_GELU_BF16_LN, NQ>`), `layernorm_kernel<8>` / `embed_stats_kernel<8>` at d = 1280;
  skinny (d = 1024: STEPS = 4 / 16, d = 1280: STEPS = 5 / 20 — GPT-2-large width) and ln_standalone.  d = 128 has no skinny form
  (K = 128 is not a multiple of 8 slices x 32): FWD_SKINNY keeps the tiles there.
* test_decode_row_counts (d = 768, short context): B in {1, 3, 8, 16} x {default, skinny, skinny_ragged} (skinny STEPS = 3 / 12),
  B = 17 with FWD_SKINNY (M > 16: the session falls back to the tile kernels, `attention_decode_kernel`).
* test_large_row_counts[d] (a seeded sample of 16 envs checked against the oracle):
    d = 768,  B = 1024: prefill C = 16 (M = 16384, ragged: qkv / fc `gemm8<128, 128, 2, 4, 2, *, 3>`, proj `gemm_bf16_glds<128, 64, 2>`,
              fc2 `gemm_bf16_glds<128, 64, 2>`); decode M = 1024: qkv / fc `gemm8<128, 128, 4, 4, 3, *, 3>`, proj `glds<64, 64, 4>`, fc2
              `gemm8<64, 64, 4, 2, 4>`
    d = 1024, B = 1024: the same at NQ = 4
    d = 1280, B = 1700: decode qkv / fc `gemm8<128, 128, 4, 4, 3, *, 5>`, proj `gemm_bf16_glds<64, 64, 3, EPI_RESID_F32_STATS>` (26.6 k
              tiles > 512); B = 480: qkv `glds<64, 64, 4, EPI_BF16_LN, 5>`, fc `glds<64, 64, 3, EPI_GELU_BF16_LN, 5>` (560 tiles);
              prefill M >= 2048 `gemm8<128, 128, 2, 4, 2, *, 5>`
    d = 128,  B = 1024: NQ = 1 (qkv N = 384: fewer than 128 128x128 tiles, so `glds<64, 64, 4>` at M = 1024; prefill `glds<128, 64, 2>`)
  Not reachable by the product path at these widths (no case): `glds<64, 64, 2>` of gemm_launch_ln_nq (an LN consumer with M >= 512
  and > 768 64x64 tiles always qualifies for the 8-wave tile; a residual producer reaches > 768 tiles only at M >= 2048).
* test_prefix_paths (d = 768): `attach_prefix_from` with group True / False (`attention_decode_kernel<4, true>`, prompt rows longer than
  128, idx = -1) and with FWD_SKINNY (`attention_decode_split_kernel<4, true>`); `broadcast_prefix_from` (n_shared header rows read from
  env 0) followed by decode steps and `set_len` below the header.
* test_f32_engine_long_context (`GPT2EngineF32`, d = 768, 12 heads, matmul f32 / bf16x3): the long schedule through
  `attn_chunk_f32_kernel<16 | 8>` and `attn_decode_f32_kernel<8>`, K / V cache and last_hidden at the tolerances of
  tests/test_gpu_f32_engine.py::test_f32_engine_hidden_states_and_cache_vs_float64.

FWD_ATTN_ITEMS2 / 3, FWD_KV_FROM_GEMM and the ragged forms are asserted bit-identical to the default at long context in
tests/test_gpu_gpt2.py (test_ragged_prefill_is_bit_identical, test_indexed_prefix_attention_equals_copied_prefix).
"""
import math

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_POS = 1024
VOCAB = 1000
HEADS = {128: 2, 768: 12, 1024: 16, 1280: 20}
BIG_DIMS = ((3, 144.0), (-5, -112.0))       # (column, added magnitude) of the sharp regime; bf16-exact

# ---- bounds.  MEASURED holds the errors the first MI355X run of this module measured (the kernels are bit-reproducible run to run, so
# the worst value is that value); every bound is BOUND_FACTOR x the measured value.  Keys: case/regime/session -> values in METRICS order
# (the differential d* metrics exist for the variant sessions of the long-context and row-count cases only):
#   kv_fro / kv_row      K / V cache rows vs the oracle, worst layer
#   hid_fro / hid_row    last_hidden after every forward and all_hidden rows vs the oracle
#   dec_fro / dec_row    last_hidden after the decode forwards alone vs the oracle
#   dkv_* / dhid_* / ddec_*  the same rows, variant session vs the default session (`differential`)
METRICS = ("kv_fro", "kv_row", "hid_fro", "hid_row", "dec_fro", "dec_row", "dkv_fro", "dkv_row", "dhid_fro", "dhid_row", "ddec_fro", "ddec_row")
BOUND_FACTOR = 2.0
MEASURED = {
    "f32bf16x3/plain/f32_bf16x3": (3.75e-6, 6.69e-6, 3.18e-6, 3.71e-6, 3.28e-6, 3.40e-6),
    "f32bf16x3/sharp/f32_bf16x3": (7.37e-6, 1.66e-5, 3.25e-5, 8.93e-5, 2.83e-5, 6.84e-5),
    "f32f32/plain/f32_f32": (9.91e-7, 2.26e-6, 9.33e-7, 1.88e-6, 9.53e-7, 1.15e-6),
    "f32f32/sharp/f32_f32": (1.59e-6, 3.85e-6, 6.86e-6, 1.96e-5, 6.18e-6, 1.49e-5),
    "large1024/plain/B1024": (4.31e-3, 7.77e-3, 3.85e-3, 6.14e-3, 3.85e-3, 5.03e-3),
    "large1024/sharp/B1024": (7.34e-3, 1.76e-2, 3.66e-2, 9.51e-2, 3.80e-2, 9.51e-2),
    "large128/plain/B1024": (2.91e-3, 6.21e-3, 1.78e-3, 2.73e-3, 1.77e-3, 2.39e-3),
    "large128/sharp/B1024": (3.18e-3, 7.61e-3, 2.52e-3, 5.22e-3, 2.58e-3, 5.22e-3),
    "large1280/plain/B1700": (4.64e-3, 7.93e-3, 3.94e-3, 5.69e-3, 3.94e-3, 5.69e-3),
    "large1280/plain/B480": (4.62e-3, 7.09e-3, 3.97e-3, 6.74e-3, 3.95e-3, 6.74e-3),
    "large1280/sharp/B1700": (7.94e-3, 1.74e-2, 4.64e-2, 1.07e-1, 5.15e-2, 1.07e-1),
    "large1280/sharp/B480": (7.76e-3, 1.51e-2, 5.03e-2, 1.21e-1, 4.14e-2, 8.68e-2),
    "large768/plain/B1024": (4.05e-3, 5.95e-3, 3.34e-3, 3.76e-3, 3.32e-3, 3.60e-3),
    "large768/sharp/B1024": (6.72e-3, 1.37e-2, 2.10e-2, 4.84e-2, 2.06e-2, 4.84e-2),
    "long1024/plain/default": (3.85e-3, 6.72e-3, 3.63e-3, 6.45e-3, 3.69e-3, 5.83e-3),
    "long1024/plain/skinny": (3.85e-3, 6.72e-3, 3.63e-3, 6.45e-3, 3.68e-3, 5.83e-3, 7.50e-5, 6.32e-3, 6.40e-4, 5.07e-3, 1.69e-3, 5.07e-3),
    "long1024/plain/ln_standalone": (3.16e-3, 6.41e-3, 3.06e-3, 5.31e-3, 3.07e-3, 4.29e-3, 4.32e-3, 8.69e-3, 4.64e-3, 7.85e-3, 4.71e-3, 7.24e-3),
    "long1024/sharp/default": (9.62e-3, 2.04e-2, 5.02e-2, 1.41e-1, 5.57e-2, 1.20e-1),
    "long1024/sharp/skinny": (9.62e-3, 2.04e-2, 5.02e-2, 1.41e-1, 5.56e-2, 1.20e-1, 9.27e-5, 5.88e-3, 1.15e-3, 1.05e-2, 3.06e-3, 1.05e-2),
    "long1024/sharp/ln_standalone": (7.82e-3, 1.69e-2, 4.12e-2, 1.45e-1, 4.91e-2, 1.14e-1, 1.10e-2, 2.67e-2, 6.47e-2, 2.06e-1, 7.54e-2, 2.06e-1),
    "long128/plain/default": (2.91e-3, 6.50e-3, 1.77e-3, 2.69e-3, 1.77e-3, 2.57e-3),
    "long128/plain/ln_standalone": (2.38e-3, 5.79e-3, 1.72e-3, 2.74e-3, 1.71e-3, 2.55e-3, 3.56e-3, 7.84e-3, 1.80e-3, 5.31e-3, 1.82e-3, 4.95e-3),
    "long128/sharp/default": (3.26e-3, 9.83e-3, 2.79e-3, 6.95e-3, 2.78e-3, 4.71e-3),
    "long128/sharp/ln_standalone": (2.73e-3, 7.03e-3, 2.55e-3, 5.56e-3, 2.57e-3, 5.40e-3, 3.86e-3, 1.15e-2, 3.53e-3, 8.87e-3, 3.53e-3, 8.87e-3),
    "long1280/plain/default": (4.05e-3, 6.98e-3, 3.66e-3, 6.24e-3, 3.71e-3, 5.74e-3),
    "long1280/plain/skinny": (4.05e-3, 6.98e-3, 3.66e-3, 6.24e-3, 3.71e-3, 5.74e-3, 1.15e-4, 7.40e-3, 6.72e-4, 5.29e-3, 1.78e-3, 5.29e-3),
    "long1280/plain/ln_standalone": (3.36e-3, 6.21e-3, 3.06e-3, 5.32e-3, 3.09e-3, 4.95e-3, 4.45e-3, 7.81e-3, 4.67e-3, 7.77e-3, 4.76e-3, 7.77e-3),
    "long1280/sharp/default": (1.03e-2, 2.16e-2, 7.24e-2, 2.05e-1, 7.24e-2, 1.69e-1),
    "long1280/sharp/skinny": (1.03e-2, 2.16e-2, 7.25e-2, 2.05e-1, 7.30e-2, 1.72e-1, 1.81e-4, 7.40e-3, 2.97e-3, 2.70e-2, 7.86e-3, 2.70e-2),
    "long1280/sharp/ln_standalone": (8.40e-3, 1.72e-2, 5.46e-2, 1.52e-1, 6.05e-2, 1.43e-1, 1.22e-2, 2.98e-2, 8.75e-2, 2.63e-1, 8.20e-2, 1.51e-1),
    "long768/plain/default": (3.67e-3, 6.79e-3, 3.26e-3, 4.94e-3, 3.24e-3, 4.29e-3),
    "long768/plain/skinny": (3.67e-3, 6.79e-3, 3.26e-3, 4.94e-3, 3.24e-3, 4.29e-3, 1.08e-4, 5.02e-3, 5.51e-4, 6.84e-3, 1.32e-3, 6.84e-3),
    "long768/plain/skinny_ragged": (3.67e-3, 6.79e-3, 3.26e-3, 4.94e-3, 3.24e-3, 4.29e-3, 1.08e-4, 5.02e-3, 5.51e-4, 6.84e-3, 1.32e-3, 6.84e-3),
    "long768/plain/valu": (3.67e-3, 6.79e-3, 3.26e-3, 4.87e-3, 3.24e-3, 4.29e-3, 4.76e-4, 7.69e-3, 2.22e-3, 7.75e-3, 1.79e-3, 7.29e-3),
    "long768/plain/ln_standalone": (3.04e-3, 5.96e-3, 2.77e-3, 4.71e-3, 2.77e-3, 4.71e-3, 4.18e-3, 9.56e-3, 4.13e-3, 7.75e-3, 4.11e-3, 7.63e-3),
    "long768/sharp/default": (8.54e-3, 2.54e-2, 3.19e-2, 1.02e-1, 3.04e-2, 7.38e-2),
    "long768/sharp/skinny": (8.54e-3, 2.54e-2, 3.19e-2, 1.02e-1, 3.02e-2, 7.44e-2, 1.30e-4, 5.15e-3, 9.83e-4, 1.39e-2, 2.34e-3, 1.39e-2),
    "long768/sharp/skinny_ragged": (8.54e-3, 2.54e-2, 3.19e-2, 1.02e-1, 3.02e-2, 7.44e-2, 1.30e-4, 5.15e-3, 9.83e-4, 1.39e-2, 2.34e-3, 1.39e-2),
    "long768/sharp/valu": (8.54e-3, 2.54e-2, 3.19e-2, 1.02e-1, 3.02e-2, 7.44e-2, 4.93e-4, 7.57e-3, 5.39e-3, 2.09e-2, 3.72e-3, 1.26e-2),
    "long768/sharp/ln_standalone": (6.83e-3, 1.54e-2, 2.46e-2, 7.34e-2, 2.43e-2, 6.95e-2, 9.26e-3, 2.59e-2, 3.85e-2, 1.15e-1, 3.75e-2, 1.03e-1),
    "prefix/plain/attach_group": (3.89e-3, 5.50e-3, 3.39e-3, 3.87e-3, 3.39e-3, 3.87e-3),
    "prefix/plain/attach_nogroup": (3.89e-3, 5.50e-3, 3.39e-3, 3.87e-3, 3.39e-3, 3.87e-3),
    "prefix/plain/attach_skinny": (3.90e-3, 5.50e-3, 3.39e-3, 3.87e-3, 3.39e-3, 3.87e-3),
    "prefix/plain/prefix_src": (3.70e-3, 6.74e-3, 3.24e-3, 5.12e-3, 0, 0),
    "prefix/plain/broadcast_setlen": (3.75e-3, 7.37e-3, 3.20e-3, 3.92e-3, 3.19e-3, 3.92e-3),
    "prefix/sharp/attach_group": (7.52e-3, 1.24e-2, 2.43e-2, 6.17e-2, 2.43e-2, 6.17e-2),
    "prefix/sharp/attach_nogroup": (7.52e-3, 1.24e-2, 2.43e-2, 6.17e-2, 2.43e-2, 6.17e-2),
    "prefix/sharp/attach_skinny": (7.52e-3, 1.24e-2, 2.43e-2, 5.87e-2, 2.43e-2, 5.87e-2),
    "prefix/sharp/prefix_src": (8.18e-3, 1.57e-2, 3.62e-2, 8.73e-2, 0, 0),
    "prefix/sharp/broadcast_setlen": (7.96e-3, 1.78e-2, 3.14e-2, 5.54e-2, 3.50e-2, 5.54e-2),
    "rows/plain/B1_default": (3.88e-3, 6.32e-3, 3.25e-3, 3.08e-3, 3.20e-3, 2.86e-3),
    "rows/plain/B1_skinny": (3.88e-3, 6.32e-3, 3.25e-3, 3.08e-3, 3.20e-3, 2.86e-3, 9.01e-6, 1.14e-3, 0, 0, 0, 0),
    "rows/plain/B1_skinny_ragged": (3.88e-3, 6.32e-3, 3.25e-3, 3.08e-3, 3.20e-3, 2.86e-3, 9.01e-6, 1.14e-3, 0, 0, 0, 0),
    "rows/plain/B3_default": (3.89e-3, 6.22e-3, 3.34e-3, 4.43e-3, 3.27e-3, 4.01e-3),
    "rows/plain/B3_skinny": (3.89e-3, 6.22e-3, 3.34e-3, 4.43e-3, 3.27e-3, 4.01e-3, 3.57e-5, 2.38e-3, 5.82e-4, 6.25e-3, 8.96e-4, 6.25e-3),
    "rows/plain/B3_skinny_ragged": (3.89e-3, 6.22e-3, 3.34e-3, 4.43e-3, 3.27e-3, 4.01e-3, 3.57e-5, 2.38e-3, 5.82e-4, 6.25e-3, 8.96e-4, 6.25e-3),
    "rows/plain/B8_default": (3.85e-3, 6.64e-3, 3.30e-3, 4.53e-3, 3.23e-3, 3.95e-3),
    "rows/plain/B8_skinny": (3.85e-3, 6.64e-3, 3.31e-3, 4.53e-3, 3.25e-3, 3.95e-3, 1.37e-4, 4.78e-3, 6.80e-4, 3.70e-3, 1.05e-3, 3.70e-3),
    "rows/plain/B8_skinny_ragged": (3.85e-3, 6.64e-3, 3.31e-3, 4.53e-3, 3.25e-3, 3.95e-3, 1.37e-4, 4.78e-3, 6.80e-4, 3.70e-3, 1.05e-3, 3.70e-3),
    "rows/plain/B16_default": (3.88e-3, 6.35e-3, 3.28e-3, 4.69e-3, 3.23e-3, 4.02e-3),
    "rows/plain/B16_skinny": (3.88e-3, 6.35e-3, 3.28e-3, 4.69e-3, 3.23e-3, 4.02e-3, 1.37e-4, 5.12e-3, 7.00e-4, 3.92e-3, 1.11e-3, 3.92e-3),
    "rows/plain/B16_skinny_ragged": (3.88e-3, 6.35e-3, 3.28e-3, 4.69e-3, 3.23e-3, 4.02e-3, 1.37e-4, 5.12e-3, 7.00e-4, 3.92e-3, 1.11e-3, 3.92e-3),
    "rows/plain/B17_default": (3.88e-3, 6.67e-3, 3.30e-3, 4.43e-3, 3.24e-3, 4.03e-3),
    "rows/plain/B17_skinny": (3.88e-3, 6.67e-3, 3.30e-3, 4.43e-3, 3.24e-3, 4.03e-3, 0, 0, 0, 0, 0, 0),
    "rows/plain/B17_skinny_ragged": (3.88e-3, 6.67e-3, 3.30e-3, 4.43e-3, 3.24e-3, 4.03e-3, 0, 0, 0, 0, 0, 0),
    "rows/sharp/B1_default": (6.98e-3, 1.17e-2, 2.06e-2, 3.65e-2, 1.84e-2, 2.35e-2),
    "rows/sharp/B1_skinny": (6.98e-3, 1.17e-2, 2.06e-2, 3.65e-2, 1.84e-2, 2.35e-2, 2.42e-7, 7.93e-5, 4.60e-4, 2.65e-3, 7.60e-4, 2.65e-3),
    "rows/sharp/B1_skinny_ragged": (6.98e-3, 1.17e-2, 2.06e-2, 3.65e-2, 1.84e-2, 2.35e-2, 2.42e-7, 7.93e-5, 4.60e-4, 2.65e-3, 7.60e-4, 2.65e-3),
    "rows/sharp/B3_default": (7.45e-3, 1.43e-2, 2.50e-2, 4.63e-2, 2.33e-2, 3.80e-2),
    "rows/sharp/B3_skinny": (7.45e-3, 1.43e-2, 2.50e-2, 4.63e-2, 2.33e-2, 3.80e-2, 1.93e-4, 4.71e-3, 9.21e-4, 3.22e-3, 1.41e-3, 3.22e-3),
    "rows/sharp/B3_skinny_ragged": (7.45e-3, 1.43e-2, 2.50e-2, 4.63e-2, 2.33e-2, 3.80e-2, 1.93e-4, 4.71e-3, 9.21e-4, 3.22e-3, 1.41e-3, 3.22e-3),
    "rows/sharp/B8_default": (7.36e-3, 1.67e-2, 2.72e-2, 6.27e-2, 2.67e-2, 5.56e-2),
    "rows/sharp/B8_skinny": (7.36e-3, 1.67e-2, 2.73e-2, 6.27e-2, 2.67e-2, 5.56e-2, 9.77e-5, 2.79e-3, 1.19e-3, 6.41e-3, 1.89e-3, 6.41e-3),
    "rows/sharp/B8_skinny_ragged": (7.36e-3, 1.67e-2, 2.73e-2, 6.27e-2, 2.67e-2, 5.56e-2, 9.77e-5, 2.79e-3, 1.19e-3, 6.41e-3, 1.89e-3, 6.41e-3),
    "rows/sharp/B16_default": (7.46e-3, 1.97e-2, 2.95e-2, 8.41e-2, 3.11e-2, 7.20e-2),
    "rows/sharp/B16_skinny": (7.46e-3, 1.97e-2, 2.95e-2, 8.41e-2, 3.10e-2, 7.20e-2, 7.42e-5, 5.43e-3, 6.92e-4, 5.68e-3, 1.11e-3, 5.68e-3),
    "rows/sharp/B16_skinny_ragged": (7.46e-3, 1.97e-2, 2.95e-2, 8.41e-2, 3.10e-2, 7.20e-2, 7.42e-5, 5.43e-3, 6.92e-4, 5.68e-3, 1.11e-3, 5.68e-3),
    "rows/sharp/B17_default": (7.40e-3, 1.66e-2, 2.75e-2, 6.69e-2, 3.35e-2, 6.69e-2),
    "rows/sharp/B17_skinny": (7.40e-3, 1.66e-2, 2.75e-2, 6.69e-2, 3.35e-2, 6.69e-2, 0, 0, 0, 0, 0, 0),
    "rows/sharp/B17_skinny_ragged": (7.40e-3, 1.66e-2, 2.75e-2, 6.69e-2, 3.35e-2, 6.69e-2, 0, 0, 0, 0, 0, 0),
}
VARIANT_FLOOR = 2e-4        # absolute floor of err_variant <= 1.25 err_default + floor (relative-error units)


@pytest.fixture(scope="module")
def dev():
    from lmrl_gym_amd import _lib
    return _lib.require_gpu()


def _cfg(d):
    from lmrl_gym_amd.gpt2 import GPT2Config
    return GPT2Config(2, HEADS[d], d, 4 * d, VOCAB, N_POS)


def make_weights(cfg, sharp, seed=11):
    """bf16-rounded HF-layout weights of the `plain` or `sharp` regime (module docstring)."""
    from lmrl_gym_amd.gpt2 import init_hf_style_state_dict
    from oracle import gpt2 as O
    sd = init_hf_style_state_dict(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if sd[k].dim() == 1:
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)
    if sharp:
        d = cfg.d_model
        sd["wte.weight"] = sd["wte.weight"] * 16          # ordinary residual dimensions ~0.5, as in trained checkpoints
        sd["wpe.weight"] = sd["wpe.weight"] * 16
        big = torch.zeros(d, dtype=torch.bool)
        for c, v in BIG_DIMS:
            sd["wpe.weight"][:, c] += v
            big[c] = True
        gain = math.sqrt(sum(v * v for _, v in BIG_DIMS) / d) / 0.45      # restores ~unit LayerNorm outputs on the ordinary dimensions
        for k in sd:
            if k.endswith("ln_1.weight") or k.endswith("ln_2.weight") or k == "ln_f.weight":
                sd[k] = torch.where(big, torch.full_like(sd[k], 0.01), sd[k] * gain)
        s = _qk_scale(sd, cfg)
        for l in range(cfg.n_layer):
            w = sd[f"h.{l}.attn.c_attn.weight"].clone()
            w[:, : 2 * d] *= s
            sd[f"h.{l}.attn.c_attn.weight"] = w
            # attention outputs carry most of each layer's residual update: a mis-weighted cached position reaches layer l + 1's K / V rows
            sd[f"h.{l}.attn.c_proj.weight"] = sd[f"h.{l}.attn.c_proj.weight"] * 4
    return O.round_weights_to_bf16(sd)


def _layer0_qk(sd, cfg, ids, pos):
    from oracle import gpt2 as O
    sd64 = {k: sd[k].double() for k in ("wte.weight", "wpe.weight", "h.0.ln_1.weight", "h.0.ln_1.bias", "h.0.attn.c_attn.weight", "h.0.attn.c_attn.bias")}
    x = sd64["wte.weight"][ids] + sd64["wpe.weight"][pos]
    h = O.layer_norm(x, sd64["h.0.ln_1.weight"], sd64["h.0.ln_1.bias"], cfg.ln_eps)
    qkv = h @ sd64["h.0.attn.c_attn.weight"] + sd64["h.0.attn.c_attn.bias"]
    d = cfg.d_model
    return qkv[..., :d], qkv[..., d:2 * d]


def _qk_scale(sd, cfg, target=7.0):
    """Q / K column scale that gives layer 0's raw scores a standard deviation of `target` on random tokens (deterministic)."""
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, cfg.vocab, (256,), generator=g)
    pos = torch.randint(0, cfg.n_pos, (256,), generator=g)
    q, k = _layer0_qk(sd, cfg, ids, pos)
    H = cfg.n_head
    sc = torch.einsum("thd,shd->hts", q.reshape(-1, H, 64), k.reshape(-1, H, 64)) / 8
    return math.sqrt(target / float(sc.std()))


def median_top1(sd, cfg, seqs, n_query=48):
    """Median over heads and the last n_query positions of the longest checked sequences of layer 0's top-1 attention weight (oracle)."""
    tops = []
    for s in sorted(seqs, key=len)[-2:]:
        T = len(s)
        if T < 2:
            continue
        q, k = _layer0_qk(sd, cfg, torch.tensor(s), torch.arange(T))
        H = cfg.n_head
        q, k = q.reshape(T, H, 64), k.reshape(T, H, 64)
        for t in range(max(1, T - n_query), T):
            a = torch.einsum("hd,shd->hs", q[t], k[: t + 1]) / 8
            tops.append(a.softmax(-1).max(-1).values)
    return float(torch.cat(tops).median())


# ------------------------------------------------------------------ the oracle and the metrics
def oracle(sd, seqs, n_head, group=4):
    """float64 oracle over right-padded sequences (causal: padding never reaches a real position) -> per env (hid [T, d], K [L][T, d], V)."""
    from oracle import gpt2 as O
    out = []
    for i in range(0, len(seqs), group):
        part = seqs[i:i + group]
        T = max(1, max(len(s) for s in part))
        ids = torch.zeros(len(part), T, dtype=torch.long)
        for j, s in enumerate(part):
            ids[j, : len(s)] = torch.tensor(s, dtype=torch.long)
        _, hid, (ks, vs) = O.forward(sd, ids, n_head, dtype=torch.float64, return_hidden=True, return_kv=True)
        for j in range(len(part)):
            out.append((hid[j], [k[j] for k in ks], [v[j] for v in vs]))
    return out


def _err(got, ref):
    """(relative Frobenius error, worst per-row max-abs error / row max) of [rows, d] float64 tensors."""
    if ref.numel() == 0:
        return 0.0, 0.0
    fro = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    row = float(((got - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-6)).max())
    return fro, row


class Trace:
    """Engine outputs of one session, keyed by env and position, compared with the oracle afterwards."""

    def __init__(self, B):
        self.seqs = [[] for _ in range(B)]
        self.hid = []            # (env, position, row float64, written by a decode forward)

    def metrics(self, kv, ref, envs, n_layer, first_pos=None):
        """kv: [2 n_layer, B, tmax, d] float64 (K of layer l at 2 l, V at 2 l + 1); ref: oracle() of [seqs[b] for b in envs]."""
        m = {}
        r = {b: i for i, b in enumerate(envs)}
        kv_fro = kv_row = 0.0
        for l in range(n_layer):
            for w in (0, 1):
                got, want = [], []
                for b in envs:
                    p0 = 0 if first_pos is None else int(first_pos[b])
                    n = len(self.seqs[b])
                    got.append(kv[2 * l + w, b, p0:n].double())
                    want.append((ref[r[b]][1 + w][l])[p0:n])
                f, rw = _err(torch.cat(got), torch.cat(want))
                m[f"{'kv'[w]}{l}_fro"], m[f"{'kv'[w]}{l}_row"] = f, rw
                kv_fro, kv_row = max(kv_fro, f), max(kv_row, rw)
        m.update(kv_fro=kv_fro, kv_row=kv_row)
        for name, sel in (("hid", lambda dec: True), ("dec", lambda dec: dec)):     # dec: the decode forwards' rows alone
            rows = [(h, ref[r[b]][0][p]) for b, p, h, dec in self.hid if b in r and sel(dec)]
            f, rw = _err(torch.stack([a for a, _ in rows]), torch.stack([b for _, b in rows])) if rows else (0.0, 0.0)
            m[name + "_fro"], m[name + "_row"] = f, rw
        return m


def differential(tr, kv, tr0, kv0, envs, n_layer):
    """A variant session against the default one on the same tokens (two independent kernel paths: far below the oracle's bf16 noise).
    dkv_* over every live K / V row of every layer, dhid_* over every recorded hidden-state row, ddec_* over the decode forwards' rows."""
    got, want = [], []
    for b in envs:
        n = len(tr0.seqs[b])
        got.append(kv[: 2 * n_layer, b, :n].double().reshape(-1, kv.shape[-1]))
        want.append(kv0[: 2 * n_layer, b, :n].double().reshape(-1, kv.shape[-1]))
    m = dict(zip(("dkv_fro", "dkv_row"), _err(torch.cat(got), torch.cat(want))))
    assert [(b, p) for b, p, _, _ in tr.hid] == [(b, p) for b, p, _, _ in tr0.hid]
    m.update(zip(("dhid_fro", "dhid_row"), _err(torch.stack([h for _, _, h, _ in tr.hid]), torch.stack([h for _, _, h, _ in tr0.hid]))))
    m.update(zip(("ddec_fro", "ddec_row"), _err(torch.stack([h for _, _, h, dec in tr.hid if dec]), torch.stack([h for _, _, h, dec in tr0.hid if dec]))))
    return m


def drive(ses, plan, seed, vocab, dev, trace=None, all_hidden_steps=(), f32=False):
    """Run `plan` = [(C, cnts)] on `ses` with seeded tokens (the same tokens for every session driven with the same seed); records
    last_hidden of every live env after every forward and all_hidden rows of the steps listed; checks lengths and the untouched state of
    envs with cnt = 0 (and, on an all-zero step, of the whole cache)."""
    B = ses.B
    trace = trace or Trace(B)
    rng = np.random.RandomState(seed)
    d = ses.last_hidden.shape[1]
    for i, (C, cnts) in enumerate(plan):
        cnts = np.asarray(cnts, dtype=np.int32)
        toks = rng.randint(0, vocab, size=(B, C)).astype(np.int32)
        allh = None
        if i in all_hidden_steps:
            allh = torch.zeros(B * C, d, dtype=torch.float32 if f32 else torch.bfloat16, device=dev)
        before_h = ses.last_hidden.clone()
        before_kv = ses.kv.clone() if not cnts.any() else None
        started = np.array([len(s) > 0 for s in trace.seqs])
        after = max(len(s) + int(c) for s, c in zip(trace.seqs, cnts))
        ses.forward(torch.from_numpy(toks.reshape(-1)).to(dev), torch.from_numpy(cnts).to(dev), C, all_hidden=allh, len_bound_after=after)
        lh = ses.last_hidden.double().cpu()
        for b in range(B):
            c = int(cnts[b])
            if c == 0:
                continue
            p0 = len(trace.seqs[b])
            trace.seqs[b] += toks[b, :c].tolist()
            trace.hid.append((b, p0 + c - 1, lh[b], C == 1))
            if allh is not None:
                ah = allh.double().cpu().reshape(B, C, d)
                for j in range(c):
                    trace.hid.append((b, p0 + j, ah[b, j], False))
        assert ses.len.cpu().tolist() == [len(s) for s in trace.seqs], i
        idle = torch.from_numpy((cnts == 0) & started).to(dev)       # (an env that never had a token has no hidden state to keep)
        assert torch.equal(ses.last_hidden[idle], before_h[idle]), i
        if before_kv is not None:
            assert torch.equal(ses.kv, before_kv), i
    return trace


def bf16_kv(ses, n_layer):
    d = ses.last_hidden.shape[1]
    return ses.kv.view(torch.bfloat16).view(2 * n_layer, ses.B, ses.tmax, d).cpu()


def long_plan(starts, decode_live):
    """Prefill every env to starts[b] (an 8-token chunk with ragged counts, 16-token chunks, a closing 8-token chunk), then one decode
    step per row of decode_live (0 / 1 per env)."""
    starts = np.asarray(starts)
    B = len(starts)
    ln = np.minimum(starts, 3 + np.arange(B) % 6)
    plan = [(8, ln.copy())]
    while (ln < starts - 8).any():
        c = np.clip(starts - 8 - ln, 0, 16)
        plan.append((16, c))
        ln = ln + c
    plan.append((8, starts - ln))
    for row in decode_live:
        plan.append((1, np.asarray(row)))
    return plan


def _assert_bounds(key, m):
    meas = MEASURED[key]
    assert len(meas) == sum(k in m for k in METRICS), key
    for name, v in zip(METRICS, meas):
        assert m[name] <= BOUND_FACTOR * v, (key, name, m[name], BOUND_FACTOR * v)


def _assert_variant(name, m, m0):
    for k in ("kv_fro", "hid_fro", "dec_fro"):
        assert m[k] <= 1.25 * m0[k] + VARIANT_FLOOR, (name, k, m[k], m0[k])


def _cached_oracle(cache, key, sd, seqs, n_head):
    if key not in cache:
        cache[key] = oracle(sd, seqs, n_head)
    return cache[key]


# ------------------------------------------------------------------ cases (each returns {session name: metrics})
def _variants(d):
    from lmrl_gym_amd.gpt2 import FWD_ATTN_VALU, FWD_LN_STANDALONE, FWD_RAGGED_ALWAYS, FWD_SKINNY
    v = {"default": 0, "skinny": FWD_SKINNY, "skinny_ragged": FWD_SKINNY | FWD_RAGGED_ALWAYS, "valu": FWD_ATTN_VALU, "ln_standalone": FWD_LN_STANDALONE}
    if d != 768:
        v = {k: v[k] for k in (("default", "ln_standalone") if d == 128 else ("default", "skinny", "ln_standalone"))}
    return v


LONG_STARTS_768 = [0, 1, 7, 31, 95, 127, 255, 511, 1000, 1016, 30, 200]
LONG_STARTS_W = [0, 129, 600, 1016]


def _long_decode_rows(B, far):
    """Decode steps: everyone, finished rows between live ones, an all-zero step, then everyone six times (the env `far` decodes in all
    eight live steps: 1016 -> 1024 = tmax)."""
    gap = [1 if (b % 3 != 1 or b == far) else 0 for b in range(B)]
    return [[1] * B, gap, [0] * B] + [[1] * B] * 6


def case_long(dev, d, sharp, seed=3):
    from lmrl_gym_amd.gpt2 import GPT2Engine
    cfg = _cfg(d)
    sd = make_weights(cfg, sharp)
    eng = GPT2Engine(cfg, sd, dev)
    starts = LONG_STARTS_768 if d == 768 else LONG_STARTS_W
    B = len(starts)
    dec = _long_decode_rows(B, starts.index(1016))
    plan = long_plan(starts, dec)
    res, ref, seqs = {}, None, None
    for name, flags in _variants(d).items():      # "default" first: its token sequences feed the one oracle pass
        ses = eng.session(B, N_POS, flags=flags)
        ses.reset()
        tr = drive(ses, plan, seed, cfg.vocab, dev, all_hidden_steps=(1, len(plan) - len(dec) - 1))
        kv = bf16_kv(ses, cfg.n_layer)
        if ref is None:
            seqs, tr0, kv0 = tr.seqs, tr, kv
            assert max(len(s) for s in seqs) == N_POS and min(len(s) for s in seqs) >= 3
            ref = oracle(sd, seqs, cfg.n_head)
        assert tr.seqs == seqs
        res[name] = tr.metrics(kv, ref, list(range(B)), cfg.n_layer)
        if name != "default":
            res[name].update(differential(tr, kv, tr0, kv0, list(range(B)), cfg.n_layer))
        del ses
    res["default"]["top1"] = median_top1(sd, cfg, seqs)
    return res


def case_rows_small(dev, sharp, seed=4):
    from lmrl_gym_amd.gpt2 import FWD_RAGGED_ALWAYS, FWD_SKINNY, GPT2Engine
    cfg = _cfg(768)
    sd = make_weights(cfg, sharp)
    eng = GPT2Engine(cfg, sd, dev)
    res = {}
    for B in (1, 3, 8, 16, 17):
        g = np.random.RandomState(B)
        pre = g.randint(20, 60, size=B)
        pre[0] = 45
        plan = long_plan(pre, [[1] * B, [1 if b % 4 != 2 else 0 for b in range(B)], [1] * B])
        variants = {"default": 0, "skinny": FWD_SKINNY, "skinny_ragged": FWD_SKINNY | FWD_RAGGED_ALWAYS}
        ref = None
        for name, flags in variants.items():
            ses = eng.session(B, 64, flags=flags)
            ses.reset()
            tr = drive(ses, plan, seed + B, cfg.vocab, dev)
            kv = bf16_kv(ses, cfg.n_layer)
            if ref is None:
                seqs, tr0, kv0 = tr.seqs, tr, kv
                ref = oracle(sd, seqs, cfg.n_head, group=17)
            assert tr.seqs == seqs
            res[f"B{B}_{name}"] = tr.metrics(kv, ref, list(range(B)), cfg.n_layer)
            if name != "default":
                res[f"B{B}_{name}"].update(differential(tr, kv, tr0, kv0, list(range(B)), cfg.n_layer))
    return res


LARGE_B = {128: (1024,), 768: (1024,), 1024: (1024,), 1280: (1700, 480)}


def case_rows_large(dev, d, sharp, seed=5):
    from lmrl_gym_amd.gpt2 import GPT2Engine
    cfg = _cfg(d)
    sd = make_weights(cfg, sharp)
    eng = GPT2Engine(cfg, sd, dev)
    res = {}
    for B in LARGE_B[d]:
        g = np.random.RandomState(B + d)
        pre = g.randint(9, 17, size=B)
        pre[:3] = (16, 9, 13)
        plan = [(16, pre), (1, np.ones(B, dtype=int)), (1, (g.rand(B) < 0.8).astype(int))]
        ses = eng.session(B, 24)
        ses.reset()
        tr = drive(ses, plan, seed + B, cfg.vocab, dev)
        envs = sorted(set(g.choice(B, 13, replace=False).tolist()) | {0, 1, B - 1})
        ref = oracle(sd, [tr.seqs[b] for b in envs], cfg.n_head, group=16)
        res[f"B{B}"] = tr.metrics(bf16_kv(ses, cfg.n_layer), ref, envs, cfg.n_layer)
        del ses
    return res


def case_prefix(dev, sharp, seed=6):
    """attach_prefix_from (group True / False, and under FWD_SKINNY), broadcast_prefix_from + set_len below the header."""
    from lmrl_gym_amd.gpt2 import FWD_SKINNY, GPT2Engine
    cfg = _cfg(768)
    sd = make_weights(cfg, sharp)
    eng = GPT2Engine(cfg, sd, dev)
    rng = np.random.RandomState(seed)
    res = {}
    # -- prompt-prefix session: 3 prompts of 300 / 129 / 1 tokens
    R, cap, tmax = 3, 320, 340
    src = eng.session(R, cap)
    src.reset()
    plens = np.array([300, 129, 1])
    src_tr = drive(src, long_plan(plens, []), seed, cfg.vocab, dev)
    idx_h = np.array([0, 1, -1, 2, 0, 1, 2, 0], dtype=np.int32)
    B = len(idx_h)
    idx = torch.from_numpy(idx_h).to(dev)
    for name, flags, group in (("attach_group", 0, True), ("attach_nogroup", 0, False), ("attach_skinny", FWD_SKINNY, True)):
        ses = eng.session(B, tmax, flags=flags)
        ses.reset()
        ses.attach_prefix_from(src, idx, cap, group=group)
        tr = Trace(B)
        tr.seqs = [list(src_tr.seqs[i]) if i >= 0 else [] for i in idx_h]
        n0 = np.array([len(s) for s in tr.seqs])
        drive(ses, [(1, np.ones(B, dtype=int)), (1, [1, 0, 1, 1, 0, 1, 1, 1]), (1, np.ones(B, dtype=int))], seed + 1, cfg.vocab, dev, trace=tr)
        ref = oracle(sd, tr.seqs, cfg.n_head)
        res[name] = tr.metrics(bf16_kv(ses, cfg.n_layer), ref, list(range(B)), cfg.n_layer, first_pos=n0)
    ref = oracle(sd, src_tr.seqs, cfg.n_head)
    res["prefix_src"] = src_tr.metrics(bf16_kv(src, cfg.n_layer), ref, list(range(R)), cfg.n_layer)
    # -- broadcast header of 200 tokens (n_shared = 200), decode, then set_len below the header and continue
    hdr = eng.session(1, 208)
    hdr.reset()
    h_tr = drive(hdr, long_plan([200], []), seed + 2, cfg.vocab, dev)
    B = 5
    ses = eng.session(B, 400)
    ses.reset()
    ses.broadcast_prefix_from(hdr, 200)
    assert ses.shared_prefix == 200
    tr = Trace(B)
    tr.seqs = [list(h_tr.seqs[0]) for _ in range(B)]
    drive(ses, [(1, np.ones(B, dtype=int)), (1, [1, 0, 1, 1, 1]), (8, [8, 3, 0, 8, 5])], seed + 3, cfg.vocab, dev, trace=tr)
    lens = np.array([150, 0, 199, 37, 207], dtype=np.int32)
    ses.set_len(lens)
    tr.seqs = [s[:n] for s, n in zip(tr.seqs, lens)]
    tr.hid = [e for e in tr.hid if e[1] < lens[e[0]]]
    drive(ses, [(16, [16, 16, 9, 16, 2]), (1, np.ones(B, dtype=int)), (1, [1, 1, 0, 1, 1])], seed + 4, cfg.vocab, dev, trace=tr)
    ref = oracle(sd, tr.seqs, cfg.n_head)
    res["broadcast_setlen"] = tr.metrics(bf16_kv(ses, cfg.n_layer), ref, list(range(B)), cfg.n_layer)
    return res


def case_f32(dev, matmul, sharp, seed=7, _oracle_cache={}):
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    cfg = _cfg(768)
    sd = make_weights(cfg, sharp)
    eng = GPT2EngineF32(cfg, sd, dev, matmul=matmul)
    starts = LONG_STARTS_W
    B = len(starts)
    plan = long_plan(starts, _long_decode_rows(B, starts.index(1016)))
    ses = eng.session(B, N_POS)
    ses.reset()
    tr = drive(ses, plan, seed, cfg.vocab, dev, f32=True)
    ref = _cached_oracle(_oracle_cache, sharp, sd, tr.seqs, cfg.n_head)
    kv = ses.kv.reshape(2 * cfg.n_layer, B, N_POS, cfg.d_model).cpu()      # [layer][K | V][B][tmax][d]
    m = tr.metrics(kv, ref, list(range(B)), cfg.n_layer)
    # the tolerance form of test_f32_engine_hidden_states_and_cache_vs_float64: max-abs <= tol * max(1, |ref| max), per row
    worst = 0.0
    r = dict(zip(range(B), ref))
    for b, p, h, _ in tr.hid:
        want = r[b][0][p]
        worst = max(worst, float((h - want).abs().max()) / max(1.0, float(want.abs().max())))
    m["hid_abs"] = worst
    return {"f32_" + matmul: m}


# ------------------------------------------------------------------ tests
NON_IDENTICAL = ("skinny", "skinny_ragged", "valu", "ln_standalone")      # variants held to err <= 1.25 err_default + floor


def _check(case, regime, res):
    if regime == "sharp" and "top1" in res.get("default", {}):
        assert res["default"]["top1"] >= 0.5, res["default"]["top1"]          # the peaked-attention regime holds
    for name, m in res.items():
        _assert_bounds(f"{case}/{regime}/{name}", m)
        var, ref_name = name, "default"
        if name.startswith("B") and "_" in name:          # row-count cases: B<n>_<variant> against B<n>_default
            base, var = name.split("_", 1)
            ref_name = base + "_default"
        if var in NON_IDENTICAL and ref_name in res:
            _assert_variant(f"{case}/{regime}/{name}", m, res[ref_name])


@pytest.mark.parametrize("regime", ["plain", "sharp"])
def test_long_context_d768(dev, regime):
    _check("long768", regime, case_long(dev, 768, regime == "sharp"))


@pytest.mark.parametrize("regime", ["plain", "sharp"])
@pytest.mark.parametrize("d", [128, 1024, 1280])
def test_long_context_width(dev, d, regime):
    _check(f"long{d}", regime, case_long(dev, d, regime == "sharp"))


@pytest.mark.parametrize("regime", ["plain", "sharp"])
def test_decode_row_counts(dev, regime):
    _check("rows", regime, case_rows_small(dev, regime == "sharp"))


@pytest.mark.parametrize("regime", ["plain", "sharp"])
@pytest.mark.parametrize("d", [128, 768, 1024, 1280])
def test_large_row_counts(dev, d, regime):
    _check(f"large{d}", regime, case_rows_large(dev, d, regime == "sharp"))


@pytest.mark.parametrize("regime", ["plain", "sharp"])
def test_prefix_paths(dev, regime):
    _check("prefix", regime, case_prefix(dev, regime == "sharp"))


@pytest.mark.parametrize("regime", ["plain", "sharp"])
@pytest.mark.parametrize("matmul,tol", [("f32", 2e-5), ("bf16x3", 3e-4)])
def test_f32_engine_long_context(dev, matmul, tol, regime):
    res = case_f32(dev, matmul, regime == "sharp")
    assert res["f32_" + matmul]["hid_abs"] <= tol, res
    _check("f32" + matmul, regime, res)
