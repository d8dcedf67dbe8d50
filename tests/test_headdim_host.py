"""CPU tier: the XLS-R 1B / 2B presets, and the flop count and memory estimate at their geometry (head dims 80 / 120,
which the engine runs on the flash attention kernels: no T x T term)."""
import pytest

from suta_amd import flops as F
from suta_amd.config import PRESETS, flash_attention_applies, get_config, head_dim, num_frames, param_shapes
from suta_amd.engine import config_to_c


def test_xlsr_presets_hold_the_public_geometry():
    for name, (H, F_, d) in {"wav2vec2-xls-r-1b": (1280, 5120, 80), "wav2vec2-xls-r-2b": (1920, 7680, 120)}.items():
        cfg = get_config(name)
        assert cfg == get_config("facebook/" + name)
        assert (cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]) == (H, F_, 48)
        assert (cfg["num_attention_heads"], cfg["num_conv_pos_embedding_groups"]) == (16, 16)
        assert head_dim(cfg) == d and cfg["hidden_size"] // cfg["num_conv_pos_embedding_groups"] == d
        assert cfg["feat_extract_norm"] == "layer" and cfg["do_stable_layer_norm"] and cfg["conv_bias"]
        assert cfg["conv_dim"] == [512] * 7 and cfg["num_conv_pos_embeddings"] == 128
        c = config_to_c(cfg)
        assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads) == (H, 48, 16)
        shapes = dict(param_shapes(cfg))
        assert shapes["wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original1"] == (H, d, 128)
        assert shapes["wav2vec2.encoder.layers.47.attention.q_proj.weight"] == (H, H)


def test_tiny_head_dim_presets():
    for name, H in (("tiny-hd80", 160), ("tiny-hd120", 240)):
        cfg = get_config(name)
        assert (cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_conv_pos_embedding_groups"]) == (H, 2, 2)
        assert (cfg["num_hidden_layers"], cfg["intermediate_size"]) == (2, 320)
        assert cfg["feat_extract_norm"] == "layer" and cfg["do_stable_layer_norm"]
        assert head_dim(cfg) == H // 2 and flash_attention_applies(cfg)


def test_a_checkpoint_config_json_still_governs(tmp_path):
    import json
    raw = dict(get_config("wav2vec2-xls-r-1b"), vocab_size=77, num_hidden_layers=3, unknown_key=1)
    (tmp_path / "config.json").write_text(json.dumps(raw))
    cfg = get_config(str(tmp_path))
    assert (cfg["hidden_size"], cfg["vocab_size"], cfg["num_hidden_layers"]) == (1280, 77, 3)
    assert "unknown_key" not in cfg


def test_num_frames_unchanged():
    """The conv stack of XLS-R is wav2vec2's: the same frame counts."""
    for n in (400, 16000, 128000, 600000):
        assert num_frames(get_config("wav2vec2-xls-r-1b"), n) == num_frames(get_config("wav2vec2-base"), n)
    assert num_frames(get_config("wav2vec2-xls-r-2b"), 128000) == 399


def test_flash_head_dims():
    assert [d for d in range(8, 200, 8) if flash_attention_applies(dict(hidden_size=d, num_attention_heads=1))] == \
        [64, 72, 80, 88, 96, 104, 112, 120, 128]
    assert not flash_attention_applies(dict(hidden_size=84, num_attention_heads=1))   # not a multiple of 8
    assert flash_attention_applies(get_config("wav2vec2-base")) and not flash_attention_applies(get_config("tiny-layer"))
    assert set(PRESETS) >= {"wav2vec2-xls-r-1b", "wav2vec2-xls-r-2b", "tiny-hd80", "tiny-hd120"}


def test_attention_flops_at_head_dim_80():
    """Hand count per layer: 16 heads x (S = Q K^T: 2 T^2 80, ctx = P V: 2 T^2 80) forward; backward dP, dV, dQ, dK:
    4 products of 2 T^2 80 per head.  Adding a layer adds exactly that plus the layer's linears."""
    cfg = get_config("wav2vec2-xls-r-1b")
    n, T, H, Fd, NH, d = 128000, 399, 1280, 5120, 16, 80
    one = dict(cfg, num_hidden_layers=1)
    two = dict(cfg, num_hidden_layers=2)
    lin = 2.0 * T * (4 * H * H + 2 * H * Fd)                      # QKV + out projection, FFN1 + FFN2
    att_f = NH * 2 * (2.0 * T * T * d)
    att_b = NH * 4 * (2.0 * T * T * d)
    assert F.forward_flops(two, n) - F.forward_flops(one, n) == pytest.approx(lin + att_f, rel=1e-12)
    assert F.backward_flops(two, n) - F.backward_flops(one, n) == pytest.approx(lin + att_b, rel=1e-12)
    G, K = 16, 128
    pos = 2.0 * T * (H // G) ** 2 * K * G                         # 16 groups of width 80, 128 taps
    zero = dict(cfg, num_hidden_layers=0)
    base0 = dict(get_config("wav2vec2-large"), num_hidden_layers=0, vocab_size=cfg["vocab_size"])
    H0 = base0["hidden_size"]
    assert F.forward_flops(zero, n) - F.forward_flops(base0, n) == pytest.approx(
        pos - 2.0 * T * (H0 // G) ** 2 * K * G + 2.0 * T * (512 + cfg["vocab_size"]) * (H - H0), rel=1e-12)


def test_memory_estimate_has_no_t2_term_on_flash_geometries():
    from suta_amd import main as M
    for name in ("wav2vec2-xls-r-1b", "wav2vec2-xls-r-2b", "wav2vec2-base", "tiny-hd80"):
        cfg = get_config(name)
        assert M.workspace_bytes_per_audio_s(cfg, utt_s=30.0) == M.workspace_bytes_per_audio_s(cfg)
    big = get_config("wav2vec2-xls-r-1b")
    assert M.workspace_bytes_per_audio_s(big) >= 50 * 4 * 48 * 14 * 1280
    # a head dim the flash kernels do not take stores P per head and layer (+ dP): NH T^2 fp32 per utterance
    tiny = get_config("tiny-layer")
    grow = M.workspace_bytes_per_audio_s(tiny, utt_s=8.0) - M.workspace_bytes_per_audio_s(tiny)
    assert grow == (tiny["num_hidden_layers"] + 1) * tiny["num_attention_heads"] * 400 * 400 * 4 / 8.0
