"""Model geometry presets (HF `Wav2Vec2Config` key names) and frame-length arithmetic.

The shapes follow the public HF configs of facebook/wav2vec2-base-960h and
facebook/wav2vec2-large-960h-lv60 ("Model shapes"); key names are the
ones `transformers.Wav2Vec2Config` uses (configuration_wav2vec2.py:165-219).
"""
from __future__ import annotations

import copy
import json
import os
from typing import List

_BASE = dict(
    hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
    vocab_size=32, conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2],
    conv_bias=False, feat_extract_norm="group", do_stable_layer_norm=False,
    num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
)

_LARGE = dict(_BASE, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
              conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True)

# XLS-R 1B / 2B (facebook/wav2vec2-xls-r-1b, -2b and their CTC fine-tunes): head dims 80 / 120, positional-conv
# groups of width 80 / 120.  vocab_size is the fine-tune's; a checkpoint directory's config.json governs.
_XLSR_1B = dict(_LARGE, hidden_size=1280, num_hidden_layers=48, num_attention_heads=16, intermediate_size=5120)
_XLSR_2B = dict(_LARGE, hidden_size=1920, num_hidden_layers=48, num_attention_heads=16, intermediate_size=7680)
# MMS (facebook/mms-1b-all, -fl102, -l1107): the XLS-R 1B body plus one attention adapter per encoder layer
# (`adapter_attn_dim`, HF Wav2Vec2AttnAdapterLayer) and one adapter file per language (main.py --target_lang).
# vocab_size 154 is quoted from memory and could not be verified offline; a checkpoint directory's config.json
# governs, and --target_lang takes the size of the language's own lm_head.
_MMS_1B = dict(_XLSR_1B, adapter_attn_dim=16, vocab_size=154)

# Tiny geometries used for the committed golden vectors (tests/golden/make_golden.py).
_TINY_GROUP = dict(_BASE, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                   conv_dim=[32] * 7, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
_TINY_LAYER = dict(_TINY_GROUP, conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True)
# head dims 80 / 120 (the XLS-R 1B / 2B head and positional-conv group widths) at test size
_TINY_HD80 = dict(_TINY_LAYER, hidden_size=160, num_attention_heads=2, num_conv_pos_embedding_groups=2,
                  intermediate_size=320)
_TINY_HD120 = dict(_TINY_HD80, hidden_size=240)
# attention adapters at test size: the MMS width 16, and a width that is no multiple of the kernels' 16-column tile
_TINY_LAYER_A16 = dict(_TINY_LAYER, adapter_attn_dim=16)
_TINY_HD80_A5 = dict(_TINY_HD80, adapter_attn_dim=5)

# Model families (`model_type` of an HF config.json; absent = wav2vec2): the state-dict prefix of each.
FAMILY_PREFIX = {"wav2vec2": "wav2vec2.", "hubert": "hubert.", "data2vec-audio": "data2vec_audio."}
FAMILY_ID = {"wav2vec2": 0, "hubert": 1, "data2vec-audio": 2}   # suta_model_family.model_family

# HuBERT (facebook/hubert-large-ls960-ft, hubert-xlarge-ls960-ft; HF HubertForCTC): the wav2vec2-large / XLS-R 1B body
# under the key prefix `hubert.`.
# data2vec-audio (facebook/data2vec-audio-base-960h, -large-960h; HF Data2VecAudioForCTC): layer-norm front end without
# conv bias, post-LN encoder, and a positional embedding of `num_conv_pos_embeddings` layers (5) of grouped
# Conv1d(k = conv_pos_kernel_size = 19) + LayerNorm(no affine) + GELU.  HF's Data2VecAudioConfig has neither
# `feat_extract_norm` nor `do_stable_layer_norm`; they are set here to what its model classes do.
# These geometries are quoted from memory and could not be verified offline; a checkpoint directory's config.json
# governs.
_HUBERT_LARGE = dict(_LARGE, model_type="hubert")
_HUBERT_XLARGE = dict(_XLSR_1B, model_type="hubert")
_D2V_BASE = dict(_BASE, model_type="data2vec-audio", feat_extract_norm="layer", do_stable_layer_norm=False,
                 conv_bias=False, num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=16)
_D2V_LARGE = dict(_D2V_BASE, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)
_TINY_D2V = dict(_TINY_GROUP, model_type="data2vec-audio", feat_extract_norm="layer", do_stable_layer_norm=False,
                 conv_bias=False, num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=4)
_TINY_D2V_EVEN = dict(_TINY_D2V, num_conv_pos_embeddings=2, conv_pos_kernel_size=4)   # even k: HF trims a frame
_TINY_HUBERT = dict(_TINY_LAYER, model_type="hubert")

PRESETS = {
    "facebook/wav2vec2-base-960h": _BASE,
    "wav2vec2-base": _BASE,
    "facebook/wav2vec2-large-960h-lv60": _LARGE,
    "facebook/wav2vec2-large-960h-lv60-self": _LARGE,
    "wav2vec2-large": _LARGE,
    "facebook/wav2vec2-xls-r-1b": _XLSR_1B,
    "wav2vec2-xls-r-1b": _XLSR_1B,
    "facebook/wav2vec2-xls-r-2b": _XLSR_2B,
    "wav2vec2-xls-r-2b": _XLSR_2B,
    "facebook/mms-1b-all": _MMS_1B,
    "mms-1b-all": _MMS_1B,
    "tiny-group": _TINY_GROUP,
    "tiny-layer": _TINY_LAYER,
    "tiny-hd80": _TINY_HD80,
    "tiny-hd120": _TINY_HD120,
    "tiny-layer-a16": _TINY_LAYER_A16,
    "tiny-hd80-a5": _TINY_HD80_A5,
    "facebook/hubert-large-ls960-ft": _HUBERT_LARGE,
    "hubert-large": _HUBERT_LARGE,
    "facebook/hubert-xlarge-ls960-ft": _HUBERT_XLARGE,
    "hubert-xlarge": _HUBERT_XLARGE,
    "facebook/data2vec-audio-base-960h": _D2V_BASE,
    "data2vec-audio-base": _D2V_BASE,
    "facebook/data2vec-audio-large-960h": _D2V_LARGE,
    "data2vec-audio-large": _D2V_LARGE,
    "tiny-d2v": _TINY_D2V,
    "tiny-d2v-even": _TINY_D2V_EVEN,
    "tiny-hubert": _TINY_HUBERT,
}


def family(cfg: dict) -> str:
    """The model family of a geometry: "wav2vec2" (no `model_type` key), "hubert" or "data2vec-audio"."""
    return cfg.get("model_type") or "wav2vec2"


def prefix(cfg: dict) -> str:
    """State-dict prefix of the family's base model (`wav2vec2.` / `hubert.` / `data2vec_audio.`)."""
    return FAMILY_PREFIX[family(cfg)]


def adapter_dim(cfg: dict) -> int:
    """Width A of the per-layer attention adapter (HF `adapter_attn_dim`), 0 for none.  HF builds the adapter only in
    the stable-LN encoder layer (`Wav2Vec2EncoderLayerStableLayerNorm`); the post-LN layer class ignores the field,
    and so do the HuBERT and data2vec-audio layer classes."""
    a = cfg.get("adapter_attn_dim")
    return int(a) if a and cfg["do_stable_layer_norm"] and family(cfg) == "wav2vec2" else 0


def head_dim(cfg: dict) -> int:
    return cfg["hidden_size"] // cfg["num_attention_heads"]


def flash_attention_applies(cfg: dict) -> bool:
    """Whether the engine runs this geometry's attention on the flash kernels (no T x T matrix stored): head dim 64,
    or 72 .. 128 in steps of 8 (csrc/attn.hip, csrc/attn_wide.hip); other head dims take the P-storing GEMM path."""
    d = head_dim(cfg)
    return d == 64 or (64 < d <= 128 and d % 8 == 0)


def get_config(name_or_path: str) -> dict:
    """Preset by model name, or a local HF checkpoint directory's config.json."""
    if name_or_path in PRESETS:
        return copy.deepcopy(PRESETS[name_or_path])
    cfg_file = os.path.join(name_or_path, "config.json")
    if os.path.isfile(cfg_file):
        with open(cfg_file) as f:
            raw = json.load(f)
        cfg = copy.deepcopy(_BASE)
        for k in cfg:
            if k in raw:
                cfg[k] = raw[k]
        if raw.get("adapter_attn_dim") is not None:   # MMS; absent or null: no adapters (the key stays out)
            cfg["adapter_attn_dim"] = int(raw["adapter_attn_dim"])
        fam = raw.get("model_type") or "wav2vec2"
        if fam not in FAMILY_PREFIX:
            raise ValueError(f"{cfg_file}: model_type '{fam}' is not one of {sorted(FAMILY_PREFIX)}")
        if fam == "hubert":
            # HubertConfig's defaults: feat_extract_norm "group", do_stable_layer_norm False, as _BASE has them
            if not raw.get("feat_proj_layer_norm", True):
                raise ValueError(f"{cfg_file}: feat_proj_layer_norm false (hubert-base: no feature-projection "
                                 "LayerNorm) is not implemented")
            if raw.get("conv_pos_batch_norm", False):
                raise ValueError(f"{cfg_file}: conv_pos_batch_norm true (BatchNorm positional conv) is not implemented")
            cfg["model_type"] = fam
        elif fam == "data2vec-audio":
            # Data2VecAudioConfig has neither key: its conv layers are all LayerNorm ones, its encoder post-LN
            cfg.update(model_type=fam, feat_extract_norm="layer", do_stable_layer_norm=False,
                       num_conv_pos_embeddings=int(raw.get("num_conv_pos_embeddings", 5)),
                       conv_pos_kernel_size=int(raw.get("conv_pos_kernel_size", 19)))
            cfg.pop("adapter_attn_dim", None)
        return cfg
    raise KeyError(f"unknown model '{name_or_path}': not a preset and no config.json found")


def frame_lengths(cfg: dict, n_samples: int) -> List[int]:
    """Conv output length per feature-encoder layer: L_i = floor((L_{i-1} - k_i)/s_i) + 1."""
    out, L = [], int(n_samples)
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        L = (L - k) // s + 1
        out.append(L)
    return out


def num_frames(cfg: dict, n_samples: int) -> int:
    return frame_lengths(cfg, n_samples)[-1]


def param_shapes(cfg: dict):
    """(name, shape) of every state_dict entry of the family's ForCTC model (Wav2Vec2ForCTC, HubertForCTC,
    Data2VecAudioForCTC), in state_dict order."""
    H, C = cfg["hidden_size"], cfg["conv_dim"]
    pfx = prefix(cfg)
    out = [(pfx + "masked_spec_embed", (H,))]
    group = cfg["feat_extract_norm"] == "group"
    for i, (c, k) in enumerate(zip(C, cfg["conv_kernel"])):
        cin = 1 if i == 0 else C[i - 1]
        b = f"{pfx}feature_extractor.conv_layers.{i}."
        out.append((b + "conv.weight", (c, cin, k)))
        if cfg["conv_bias"]:
            out.append((b + "conv.bias", (c,)))
        if (group and i == 0) or not group:
            out += [(b + "layer_norm.weight", (c,)), (b + "layer_norm.bias", (c,))]
    fp = pfx + "feature_projection."
    out += [(fp + "layer_norm.weight", (C[-1],)), (fp + "layer_norm.bias", (C[-1],)),
            (fp + "projection.weight", (H, C[-1])), (fp + "projection.bias", (H,))]
    K, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    if family(cfg) == "data2vec-audio":   # K layers of Conv1d(H, H, conv_pos_kernel_size, groups=G) with bias
        for j in range(K):
            pc = f"{pfx}encoder.pos_conv_embed.layers.{j}.conv."
            out += [(pc + "weight", (H, H // G, cfg["conv_pos_kernel_size"])), (pc + "bias", (H,))]
    else:
        pc = pfx + "encoder.pos_conv_embed.conv."
        out += [(pc + "bias", (H,)), (pc + "parametrizations.weight.original0", (1, 1, K)),
                (pc + "parametrizations.weight.original1", (H, H // G, K))]
    out += [(pfx + "encoder.layer_norm.weight", (H,)), (pfx + "encoder.layer_norm.bias", (H,))]
    F_ = cfg["intermediate_size"]
    A = adapter_dim(cfg)
    for li in range(cfg["num_hidden_layers"]):
        lp = f"{pfx}encoder.layers.{li}."
        for pr in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += [(lp + f"attention.{pr}.weight", (H, H)), (lp + f"attention.{pr}.bias", (H,))]
        out += [(lp + "layer_norm.weight", (H,)), (lp + "layer_norm.bias", (H,)),
                (lp + "feed_forward.intermediate_dense.weight", (F_, H)),
                (lp + "feed_forward.intermediate_dense.bias", (F_,)),
                (lp + "feed_forward.output_dense.weight", (H, F_)),
                (lp + "feed_forward.output_dense.bias", (H,)),
                (lp + "final_layer_norm.weight", (H,)), (lp + "final_layer_norm.bias", (H,))]
        if A:
            ap = lp + "adapter_layer."
            out += [(ap + "norm.weight", (H,)), (ap + "norm.bias", (H,)),
                    (ap + "linear_1.weight", (A, H)), (ap + "linear_1.bias", (A,)),
                    (ap + "linear_2.weight", (H, A)), (ap + "linear_2.bias", (H,))]
    out += [("lm_head.weight", (cfg["vocab_size"], H)), ("lm_head.bias", (cfg["vocab_size"],))]
    return out
