"""CPU tier: the HuBERT and data2vec-audio families in the geometry, the module walk, the weights and the C struct.

g16_family_keys.json holds HF's `Data2VecAudioForCTC` / `HubertForCTC` state_dict keys and the reference's own
collect_params output on them (tests/golden/make_golden_families.py keys).
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from suta_amd import engine as E
from suta_amd.config import (FAMILY_ID, adapter_dim, family, flash_attention_applies, get_config, head_dim,
                             param_shapes, prefix)
from suta_amd.flops import forward_flops
from suta_amd.modules import collect_params
from suta_amd.weights import remap_legacy, synth_weights

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = json.load(open(os.path.join(G, "g16_family_keys.json")))
FLAGS = ((False, True), (True, True), (False, False))


@pytest.mark.parametrize("preset", ["tiny-d2v", "tiny-hubert"])
def test_param_shapes_match_hf_state_dict(preset):
    cfg = get_config(preset)
    shapes = param_shapes(cfg)
    assert [n for n, _ in shapes] == KEYS[preset]["state_dict"]
    sd = synth_weights(cfg)
    assert list(sd) == KEYS[preset]["state_dict"]
    assert all(sd[n].shape == tuple(s) and sd[n].dtype == np.float32 for n, s in shapes)
    assert all(n.startswith(prefix(cfg)) or n.startswith("lm_head.") for n in sd)


def test_data2vec_stack_tensors():
    cfg = get_config("tiny-d2v")
    shapes = dict(param_shapes(cfg))
    for j in range(5):
        b = f"data2vec_audio.encoder.pos_conv_embed.layers.{j}.conv."
        assert shapes[b + "weight"] == (64, 16, 19) and shapes[b + "bias"] == (64,)
    assert not any("parametrizations" in n or ".conv.bias" in n and "feature_extractor" in n for n in shapes)
    even = dict(param_shapes(get_config("tiny-d2v-even")))
    assert even["data2vec_audio.encoder.pos_conv_embed.layers.1.conv.weight"] == (64, 16, 4)
    assert "data2vec_audio.encoder.pos_conv_embed.layers.2.conv.weight" not in even


@pytest.mark.parametrize("preset", ["tiny-d2v", "tiny-hubert"])
@pytest.mark.parametrize("bias_only,train_feature", FLAGS)
def test_collect_params_matches_reference(preset, bias_only, train_feature):
    printed, names = collect_params(get_config(preset), bias_only, train_feature)
    assert names == KEYS[preset][f"bias_only={bias_only},train_feature={train_feature}"]
    assert printed == KEYS[preset]["printed"]
    if preset == "tiny-d2v":   # the stack's modules print, and contribute no parameter
        assert "data2vec_audio.encoder.pos_conv_embed.layers.4.layer_norm" in printed
        assert not any("pos_conv_embed" in n for n in names)


def _write_cfg(tmp_path, name, **raw):
    d = tmp_path / name
    d.mkdir()
    json.dump(raw, open(d / "config.json", "w"))
    return str(d)


HF_COMMON = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, vocab_size=32,
                 conv_dim=[32] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2],
                 num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5)


def test_get_config_reads_data2vec_directory(tmp_path):
    # HF's Data2VecAudioConfig has neither feat_extract_norm nor do_stable_layer_norm
    d = _write_cfg(tmp_path, "d2v", model_type="data2vec-audio", conv_bias=False, num_conv_pos_embeddings=5,
                   conv_pos_kernel_size=19, **HF_COMMON)
    cfg = get_config(d)
    assert cfg == get_config("tiny-d2v")
    assert family(cfg) == "data2vec-audio" and prefix(cfg) == "data2vec_audio."
    assert cfg["feat_extract_norm"] == "layer" and cfg["do_stable_layer_norm"] is False
    assert cfg["conv_pos_kernel_size"] == 19 and cfg["num_conv_pos_embeddings"] == 5
    d = _write_cfg(tmp_path, "d2v_a", model_type="data2vec-audio", conv_bias=False, num_conv_pos_embeddings=2,
                   conv_pos_kernel_size=4, adapter_attn_dim=16, **HF_COMMON)
    cfg = get_config(d)
    assert cfg == get_config("tiny-d2v-even") and adapter_dim(cfg) == 0


def test_get_config_reads_hubert_directory(tmp_path):
    d = _write_cfg(tmp_path, "hub", model_type="hubert", conv_bias=True, feat_extract_norm="layer",
                   do_stable_layer_norm=True, num_conv_pos_embeddings=16, feat_proj_layer_norm=True,
                   conv_pos_batch_norm=False, **HF_COMMON)
    cfg = get_config(d)
    assert cfg == get_config("tiny-hubert")
    assert family(cfg) == "hubert" and prefix(cfg) == "hubert."
    assert adapter_dim(dict(cfg, adapter_attn_dim=16)) == 0   # HubertEncoderLayerStableLayerNorm builds no adapter


def test_refusals(tmp_path):
    hub = dict(HF_COMMON, model_type="hubert", conv_bias=False, num_conv_pos_embeddings=16)
    with pytest.raises(ValueError, match="feat_proj_layer_norm"):
        get_config(_write_cfg(tmp_path, "base", feat_proj_layer_norm=False, **hub))
    with pytest.raises(ValueError, match="conv_pos_batch_norm"):
        get_config(_write_cfg(tmp_path, "bn", conv_pos_batch_norm=True, **hub))
    with pytest.raises(ValueError, match="wavlm"):
        get_config(_write_cfg(tmp_path, "wavlm", **dict(hub, model_type="wavlm")))


def test_directory_without_model_type_is_unchanged(tmp_path):
    raw = dict(HF_COMMON, conv_bias=False, feat_extract_norm="group", do_stable_layer_norm=False,
               num_conv_pos_embeddings=16)
    want = get_config("tiny-group")
    assert "model_type" not in want
    assert get_config(_write_cfg(tmp_path, "plain", **raw)) == want
    assert get_config(_write_cfg(tmp_path, "named", model_type="wav2vec2", **raw)) == want
    assert family(want) == "wav2vec2" and prefix(want) == "wav2vec2."
    assert [n for n, _ in param_shapes(want)][0] == "wav2vec2.masked_spec_embed"


def test_remap_legacy_hubert_names():
    g, v = np.ones((1, 1, 16), np.float32), np.ones((64, 16, 16), np.float32)
    sd = remap_legacy({"hubert.encoder.pos_conv_embed.conv.weight_g": g,
                       "hubert.encoder.pos_conv_embed.conv.weight_v": v, "lm_head.bias": np.zeros(32, np.float32)})
    assert set(sd) == {"hubert.encoder.pos_conv_embed.conv.parametrizations.weight.original0",
                       "hubert.encoder.pos_conv_embed.conv.parametrizations.weight.original1", "lm_head.bias"}
    assert sd["hubert.encoder.pos_conv_embed.conv.parametrizations.weight.original0"] is g
    sd = remap_legacy({"wav2vec2.encoder.pos_conv_embed.conv.weight_g": g})
    assert list(sd) == ["wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original0"]


def test_presets():
    b, l = get_config("facebook/data2vec-audio-base-960h"), get_config("data2vec-audio-large")
    assert (b["hidden_size"], b["num_hidden_layers"], b["num_attention_heads"], b["intermediate_size"]) == \
        (768, 12, 12, 3072)
    assert (b["num_conv_pos_embedding_groups"], b["num_conv_pos_embeddings"], b["conv_pos_kernel_size"],
            b["conv_bias"]) == (16, 5, 19, False)
    assert (l["hidden_size"], l["num_hidden_layers"], l["num_attention_heads"], l["intermediate_size"]) == \
        (1024, 24, 16, 4096)
    assert head_dim(b) == 64 and flash_attention_applies(b) and flash_attention_applies(l)
    h, x = get_config("facebook/hubert-large-ls960-ft"), get_config("hubert-xlarge")
    assert {k: v for k, v in h.items() if k != "model_type"} == get_config("wav2vec2-large")
    assert {k: v for k, v in x.items() if k != "model_type"} == get_config("wav2vec2-xls-r-1b")
    assert head_dim(x) == 80 and flash_attention_applies(x)


def test_flops_count_the_stack():
    """The stack's five 19-tap convs: 2 * T * (H / G)^2 * G * 95 forward flops at data2vec-base."""
    b = get_config("data2vec-audio-base")
    one = dict(b, num_conv_pos_embeddings=1)
    T = 49
    assert forward_flops(b, 16000) - forward_flops(one, 16000) == 2.0 * T * 48 ** 2 * 16 * 19 * 4


def test_family_struct_rides_beside_the_config():
    """suta_model_config keeps its layout (adapter_attn_dim last); the family and the stack's kernel size travel in
    suta_model_family to suta_create_family, and the ctypes mirror has the header's fields in the header's order."""
    assert [f[0] for f in E.ModelConfigC._fields_][-1] == "adapter_attn_dim"
    header = open(os.path.join(os.path.dirname(G), "..", "include", "suta.h")).read()
    body = re.search(r"typedef struct suta_model_family \{(.*?)\} suta_model_family;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [m.group(1) for m in (re.match(r"\s*int32_t\s+(\w+)\s*$", d) for d in body.split(";")) if m]
    assert fields == [f[0] for f in E.ModelFamilyC._fields_] == ["model_family", "conv_pos_kernel_size"]
    assert ctypes.sizeof(E.ModelFamilyC) == 8
    for name, val in (("WAV2VEC2", 0), ("HUBERT", 1), ("DATA2VEC_AUDIO", 2)):
        assert re.search(rf"#define SUTA_FAMILY_{name} {val}\b", header)
    assert FAMILY_ID == {"wav2vec2": 0, "hubert": 1, "data2vec-audio": 2}
    assert "suta_create_family" in E.EXPORTS
    d2v = get_config("tiny-d2v")
    f, c = E.family_to_c(d2v), E.config_to_c(d2v)
    assert (f.model_family, f.conv_pos_kernel_size, c.num_conv_pos_embeddings) == (2, 19, 5)
    assert (c.feat_extract_norm_layer, c.do_stable_layer_norm, c.conv_bias) == (1, 0, 0)
    f = E.family_to_c(get_config("tiny-hubert"))
    assert (f.model_family, f.conv_pos_kernel_size) == (1, 0)
    f = E.family_to_c(get_config("wav2vec2-large"))
    assert (f.model_family, f.conv_pos_kernel_size) == (0, 0)
