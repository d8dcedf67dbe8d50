"""CPU tier: MMS attention adapters (`adapter_attn_dim`) in the host layers -- geometry, parameter list, module walk,
synthetic weights, FLOP count, the --target_lang overlay and vocabulary, and the ABI struct.

tests/golden/g15_adapter_keys.json holds HF's own state_dict keys and the reference's collect_params names
(tests/golden/make_golden_adapter.py)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from suta_amd import flops
from suta_amd.config import get_config, num_frames, param_shapes
from suta_amd.decode import load_vocab
from suta_amd.engine import ModelConfigC, config_to_c
from suta_amd.modules import collect_params
from suta_amd.weights import load_adapter, load_hf_checkpoint, synth_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "g15_adapter_keys.json")) as f:
    KEYS = json.load(f)
FLAGS = [(False, True), (True, True), (False, False)]   # (bias_only, train_feature)


def test_param_shapes_are_the_hf_state_dict_keys():
    cfg = get_config("tiny-layer-a16")
    assert cfg["adapter_attn_dim"] == 16
    names = [n for n, _ in param_shapes(cfg)]
    assert names == KEYS["tiny-layer-a16"]["state_dict"]
    shapes = dict(param_shapes(cfg))
    b = "wav2vec2.encoder.layers.1.adapter_layer."
    assert shapes[b + "linear_1.weight"] == (16, 64) and shapes[b + "linear_2.weight"] == (64, 16)
    assert shapes[b + "linear_1.bias"] == (16,) and shapes[b + "linear_2.bias"] == (64,) and shapes[b + "norm.weight"] == (64,)
    assert get_config("tiny-hd80-a5")["adapter_attn_dim"] == 5
    mms = get_config("facebook/mms-1b-all")
    assert (mms["hidden_size"], mms["num_hidden_layers"], mms["adapter_attn_dim"]) == (1280, 48, 16)
    assert "adapter_attn_dim" not in get_config("wav2vec2-xls-r-1b")


@pytest.mark.parametrize("bias_only,train_feature", FLAGS)
def test_collect_params_names_are_the_references(bias_only, train_feature):
    key = f"bias_only={bias_only},train_feature={train_feature}"
    _, names = collect_params(get_config("tiny-layer-a16"), bias_only, train_feature)
    assert names == KEYS["tiny-layer-a16"][key]
    want = 2 * (1 if bias_only else 2)
    assert sum(".adapter_layer.norm." in n for n in names) == want


def test_post_ln_geometry_ignores_the_field():
    """HF's post-LN encoder layer builds no adapter whatever the config says."""
    plain = get_config("tiny-group")
    cfg = dict(plain, adapter_attn_dim=16)
    assert param_shapes(cfg) == param_shapes(plain)
    assert [n for n, _ in param_shapes(cfg)] == KEYS["tiny-group+a16"]["state_dict"]
    for bias_only, train_feature in FLAGS:
        assert collect_params(cfg, bias_only, train_feature) == collect_params(plain, bias_only, train_feature)
        assert collect_params(cfg, bias_only, train_feature)[1] == \
            KEYS["tiny-group+a16"][f"bias_only={bias_only},train_feature={train_feature}"]
    assert flops.forward_flops(cfg, 16000) == flops.forward_flops(plain, 16000)


def test_get_config_reads_the_field(tmp_path):
    raw = dict(get_config("tiny-layer"), adapter_attn_dim=16, model_type="wav2vec2")
    json.dump(raw, open(tmp_path / "config.json", "w"))
    assert get_config(str(tmp_path))["adapter_attn_dim"] == 16
    json.dump(dict(raw, adapter_attn_dim=None), open(tmp_path / "config.json", "w"))
    assert "adapter_attn_dim" not in get_config(str(tmp_path))
    del raw["adapter_attn_dim"]
    json.dump(raw, open(tmp_path / "config.json", "w"))
    assert get_config(str(tmp_path)) == get_config("tiny-layer")


def test_synth_weights_keep_every_existing_draw():
    plain = synth_weights(get_config("tiny-layer"))
    sd = synth_weights(get_config("tiny-layer-a16"))
    assert set(plain) < set(sd)
    for k, v in plain.items():
        assert sd[k].tobytes() == v.tobytes(), k
    for l in range(2):
        b = f"wav2vec2.encoder.layers.{l}.adapter_layer."
        g = sd[b + "norm.weight"]
        assert np.all(np.abs(g - 1.0) <= 0.5) and np.abs(g - 1.0).max() > 0.01, "an affine around 1, not N(0, 1)"
        assert np.abs(sd[b + "norm.bias"]).max() <= 0.5
        assert sd[b + "linear_1.weight"].shape == (16, 64) and np.abs(sd[b + "linear_2.bias"]).max() < 0.2


def test_flops_count_the_adapter():
    cfg, plain = get_config("tiny-layer-a16"), get_config("tiny-layer")
    n = 32000
    T, L, H, A = num_frames(cfg, n), 2, 64, 16
    assert flops.forward_flops(cfg, n) - flops.forward_flops(plain, n) == L * T * 4 * H * A
    assert flops.backward_flops(cfg, n) - flops.backward_flops(plain, n) == L * T * 6 * H * A


def _checkpoint(root):
    """A synthetic MMS-style directory: tiny-layer-a16 (vocab 32) + adapter.xx (40 classes) + a nested vocab.json."""
    from safetensors.numpy import save_file
    cfg = get_config("tiny-layer-a16")
    sd = synth_weights(cfg)
    lang = synth_weights(dict(cfg, vocab_size=40), seed=7)
    ad = {k: v for k, v in lang.items() if ".adapter_layer." in k or k.startswith("lm_head.")}
    toks = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(ord("a") + i) for i in range(26)] + list("123456789")
    vocab = {"xx": {t: i for i, t in enumerate(toks)}, "yy": {t: i for i, t in enumerate(reversed(toks[:32]))}}
    json.dump(cfg, open(root / "config.json", "w"))
    json.dump(vocab, open(root / "vocab.json", "w"))
    save_file(sd, str(root / "model.safetensors"))
    save_file(ad, str(root / "adapter.xx.safetensors"))
    return cfg, sd, ad, vocab


def test_target_lang_overlays_the_adapter_file(tmp_path):
    from safetensors.numpy import save_file
    cfg, sd, ad, _ = _checkpoint(tmp_path)
    c2, s2 = get_config(str(tmp_path)), load_hf_checkpoint(str(tmp_path))
    assert c2["vocab_size"] == 32 and c2["adapter_attn_dim"] == 16
    load_adapter(str(tmp_path), "xx", c2, s2)
    assert c2["vocab_size"] == 40 and s2["lm_head.weight"].shape == (40, 64) and s2["lm_head.bias"].shape == (40,)
    assert dict(param_shapes(c2))["lm_head.weight"] == (40, 64)
    for k in s2:
        want = ad[k] if k in ad else sd[k]
        assert s2[k].tobytes() == want.tobytes(), k
    assert sum(".adapter_layer." in k for k in ad) == 12
    # a wrong key set raises, as HF's load_adapter does (missing and unexpected keys)
    bad = dict(ad)
    del bad["wav2vec2.encoder.layers.0.adapter_layer.linear_2.bias"]
    save_file(bad, str(tmp_path / "adapter.zz.safetensors"))
    with pytest.raises(ValueError, match="linear_2.bias"):
        load_adapter(str(tmp_path), "zz", get_config(str(tmp_path)), load_hf_checkpoint(str(tmp_path)))
    save_file(dict(ad, **{"wav2vec2.encoder.layer_norm.weight": sd["wav2vec2.encoder.layer_norm.weight"]}),
              str(tmp_path / "adapter.ww.safetensors"))
    with pytest.raises(ValueError, match="unexpected"):
        load_adapter(str(tmp_path), "ww", get_config(str(tmp_path)), load_hf_checkpoint(str(tmp_path)))
    with pytest.raises(FileNotFoundError):
        load_adapter(str(tmp_path), "qq", get_config(str(tmp_path)), load_hf_checkpoint(str(tmp_path)))


def test_target_lang_falls_back_to_the_torch_file(tmp_path):
    import torch
    cfg, sd, ad, _ = _checkpoint(tmp_path)
    os.remove(tmp_path / "adapter.xx.safetensors")
    torch.save({k: torch.from_numpy(v) for k, v in ad.items()}, str(tmp_path / "adapter.xx.bin"))
    c2, s2 = get_config(str(tmp_path)), load_hf_checkpoint(str(tmp_path))
    load_adapter(str(tmp_path), "xx", c2, s2)
    assert c2["vocab_size"] == 40 and s2["lm_head.bias"].tobytes() == ad["lm_head.bias"].tobytes()


def test_load_vocab_picks_the_language(tmp_path):
    _, _, _, vocab = _checkpoint(tmp_path)
    vx = load_vocab(str(tmp_path), target_lang="xx")
    assert len(vx.tokens) == 40 and vx.tokens[5] == "a" and vx.tokens[39] == "9"
    vy = load_vocab(str(tmp_path), target_lang="yy")
    assert len(vy.tokens) == 32 and vy.tokens[vocab["yy"]["a"]] == "a" and vy.tokens != vx.tokens[:32]
    with pytest.raises(KeyError, match="qq"):
        load_vocab(str(tmp_path), target_lang="qq")
    with pytest.raises(ValueError, match="target_lang"):
        load_vocab(str(tmp_path))
    json.dump({"target_lang": "yy"}, open(tmp_path / "tokenizer_config.json", "w"))
    assert load_vocab(str(tmp_path)).tokens == vy.tokens
    assert load_vocab(str(tmp_path), target_lang="xx").tokens == vx.tokens
    # a flat vocab.json behaves as before, with or without the argument
    os.remove(tmp_path / "tokenizer_config.json")
    json.dump(vocab["xx"], open(tmp_path / "vocab.json", "w"))
    assert load_vocab(str(tmp_path)).tokens == vx.tokens == load_vocab(str(tmp_path), target_lang="qq").tokens


def test_driver_flag_and_unchanged_experiment_name():
    from suta_amd import main as M
    a = M.build_parser().parse_args([])
    assert a.target_lang is None
    b = M.build_parser().parse_args(["--target_lang", "fra"])
    assert b.target_lang == "fra" and M.exp_name_of(a) == M.exp_name_of(b)
    assert M.build_parser(sdpl=True).parse_args(["--target_lang", "fra"]).target_lang == "fra"
    with pytest.raises(RuntimeError, match="checkpoint directory"):
        M.load_model("facebook/mms-1b-all", True, "fra")


def test_abi_struct_matches_the_header():
    src = open(os.path.join(ROOT, "include", "suta.h")).read()
    body = re.search(r"typedef struct suta_model_config \{(.*?)\} suta_model_config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n = 0
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(int32_t|float)\s+(\w+)(?:\[(\w+)\])?\s*$", decl)
        if m:
            n += 8 if m.group(3) == "SUTA_MAX_CONV" else 1
            fields.append(m.group(2))
    assert fields == [f[0] for f in ModelConfigC._fields_]
    assert fields[-1] == "adapter_attn_dim"
    assert ctypes.sizeof(ModelConfigC) == 4 * n
    assert config_to_c(get_config("tiny-layer-a16")).adapter_attn_dim == 16
    assert config_to_c(get_config("tiny-layer")).adapter_attn_dim == 0
