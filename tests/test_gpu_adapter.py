"""GPU tier: MMS attention adapters (`adapter_attn_dim`) -- the fused adapter kernels of csrc/adapter.hip in the
stable-LN encoder layers, the adapter LayerNorm's weight and bias as trainables, and the driver's --target_lang.

The reference is the reference's own forward_and_adapt on HF's Wav2Vec2ForCTC, recorded by
tests/golden/make_golden_adapter.py (g15_*); every fixture's `adapter_effect` (step-0 logits with the adapter's output
removed) is more than 100 x the tolerance applied here, so a run without the adapter cannot pass.  The tiny fixtures'
waveforms are those on which the reference's own fp32 run stays within half of logits_tol of its float64 run
(`ref_f32_err`): Adam moves an element whose gradient is of the size of its eps by a rounding-dependent fraction of lr,
and on such a waveform the recorded fp32 logits are themselves off by more than the bound.

Tolerances are the project's own for each comparison:
  * tiny models against the reference: tests/parity.logits_tol(lr); adapted tensors by tests/parity.assert_params_close
  * full-width models: atol 5e-5 on logits
  * a ragged batch against the single runs: atol 2e-5 on logits
  * bf16 mode against exact fp32: tests/parity.assert_bf16_close
"""
import ast
import json
import os
import re

import numpy as np
import pytest

from suta_amd import synth
from suta_amd.config import get_config, num_frames
from suta_amd.engine import SutaEngine, SutaHParams
from suta_amd.weights import synth_weights
from tests.parity import assert_bf16_close, assert_params_close, logits_tol

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def wide_cfg(hidden, adapter=16):
    """tests/test_gpu_headdim.py::wide_cfg (one XLS-R-shaped layer at full width, 16 heads) with the adapter."""
    cfg = get_config("wav2vec2-xls-r-1b")
    cfg.update(hidden_size=hidden, num_attention_heads=16, num_conv_pos_embedding_groups=16, num_hidden_layers=1,
               intermediate_size=256, conv_dim=[32] * 7)
    if adapter:
        cfg["adapter_attn_dim"] = adapter
    return cfg


def model(key):
    """(cfg, weights) of a preset, of wide_cfg(hidden) for 'h<hidden>', or of either without adapters ('<key>-plain')."""
    if ("model", key) not in _CACHE:
        plain = key.endswith("-plain")
        base = key[:-len("-plain")] if plain else key
        if base == "tiny-h72-a16":   # hidden 72: no multiple of the kernels' 16-column chunk (make_golden_adapter.h72_cfg)
            cfg = get_config("tiny-layer-a16")
            cfg.update(hidden_size=72, num_attention_heads=4, num_conv_pos_embedding_groups=3)
        else:
            cfg = wide_cfg(int(base[1:])) if base.startswith("h") else get_config(base)
        if plain:
            cfg.pop("adapter_attn_dim")
        _CACHE[("model", key)] = (cfg, synth_weights(cfg))
    return _CACHE[("model", key)]


def engine(key):
    if ("engine", key) not in _CACHE:
        cfg, sd = model(key)
        _CACHE[("engine", key)] = SutaEngine(cfg, sd, max_batch=2, max_samples=128000)
    eng = _CACHE[("engine", key)]
    eng.set_precision("fp32")
    return eng


def digest(sd):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def adapter_norms(cfg):
    return [f"wav2vec2.encoder.layers.{l}.adapter_layer.norm.{p}" for l in range(cfg["num_hidden_layers"])
            for p in ("weight", "bias")]


TINY_FIXTURES = [("tiny-layer-a16", "g15_adapter_tiny_layer_a16_N400.npz"),
                 ("tiny-layer-a16", "g15_adapter_tiny_layer_a16_N10960.npz"),
                 ("tiny-layer-a16", "g15_adapter_tiny_layer_a16_N32000.npz"),
                 ("tiny-hd80-a5", "g15_adapter_tiny_hd80_a5_N10960.npz"),
                 ("tiny-layer-a16", "g15_adapter_tiny_layer_a16_N10960_biasonly.npz"),
                 ("tiny-h72-a16", "g15_adapter_tiny_h72_a16_N10960.npz")]


def _run_tiny_fixture(preset, fname, precision, params=True):
    z = np.load(os.path.join(G, fname))
    cfg, sd = model(preset)
    assert digest(sd) == str(z["weights_sha256"]), "seeded weight generator drifted"
    h = ast.literal_eval(str(z["hp_json"]))
    steps = int(z["steps"])
    tol = logits_tol(h["lr"])
    assert float(z["adapter_effect"]) > 100 * tol
    # the reference's own fp32 rounding error on this waveform (against its float64 run) leaves half the bound to the
    # engine's: tests/golden/make_golden_adapter.py chooses the waveforms so
    assert float(z["ref_f32_err"].max()) <= 0.5 * tol
    eng = engine(preset)
    eng.set_precision(precision)
    hp = SutaHParams(lr=h["lr"], temp=h["temp"], em_coef=h["em"], reweight=h["rw"], non_blank=h["nb"],
                     div_coef=h["div"], train_feature=h["train_feature"], bias_only=h["bias_only"])
    try:
        logits, ids, T = eng.adapt(z["x"], steps, hp, record=list(range(steps + 1)))
        got = {k[len("final/"):]: eng.get_param(0, k[len("final/"):]) for k in z.files if k.startswith("final/")}
    finally:
        eng.set_precision("fp32")
    ref = z["logits"]
    assert T == ref.shape[1]
    for i in range(steps + 1):
        print(f"{fname} {precision} step {i}: max |engine - reference| = {float(np.abs(logits[i][0] - ref[i]).max()):.3g}")
    for i in range(steps + 1):
        np.testing.assert_allclose(logits[i][0], ref[i], rtol=0, atol=tol, err_msg=f"{fname} step {i}")
        np.testing.assert_array_equal(ids[i][0], logits[i][0].argmax(-1))
    if not params:
        return
    names = adapter_norms(cfg)
    assert set(names) <= set(got) or h["bias_only"]
    for name, v in got.items():
        assert_params_close(v, z["final/" + name], h["lr"], steps, name=name)
    if h["bias_only"]:   # the adapter LayerNorm's weight stays frozen, its bias moves
        for l in range(cfg["num_hidden_layers"]):
            b = f"wav2vec2.encoder.layers.{l}.adapter_layer.norm."
            assert np.array_equal(eng.get_param(0, b + "weight"), sd[b + "weight"])
            assert b + "bias" in got and not np.array_equal(got[b + "bias"], sd[b + "bias"])


@pytest.mark.parametrize("preset,fname", TINY_FIXTURES)
def test_tiny_adapter_matches_reference(preset, fname):
    """4 SUTA steps at lr 5e-4 on HF's model with adapters (T = 1, 34, 99; A = 16 and A = 5, padded to the MFMA's 16
    columns; --bias_only; hidden 72, whose last 16-column chunk is half empty): logits of every step, the adapted
    tensors (the adapter LayerNorms among them), greedy ids."""
    _run_tiny_fixture(preset, fname, "fp32")


@pytest.mark.parametrize("preset,fname", TINY_FIXTURES)
def test_split_bf16_mode_matches_reference(preset, fname):
    """The same fixtures with the GEMMs in the fp32-accurate 3-way bf16 split (the adapter kernels are the same exact
    fp32 in every mode): logits of every step within logits_tol, greedy ids."""
    _run_tiny_fixture(preset, fname, "fp32-split-bf16", params=False)


@pytest.mark.parametrize("hidden", [1024, 1280, 2048])
def test_full_width_adapter_matches_reference(hidden):
    """One full-width layer (4 waves per row tile at 1024, 8 at 1280 and 2048) against the reference, 2 steps."""
    z = np.load(os.path.join(G, f"g15_adapter_h{hidden}_a16_N32000.npz"))
    cfg, sd = model(f"h{hidden}")
    assert digest(sd) == str(z["weights_sha256"]), "seeded weight generator drifted"
    assert float(z["adapter_effect"]) > 100 * 5e-5
    n, seed = (int(v) for v in z["wave"])
    logits, ids, T = engine(f"h{hidden}").adapt(synth.wave(n, seed), 2, SutaHParams(), record=[0, 1, 2])
    for r in (0, 1, 2):
        print(f"hidden {hidden} step {r}: max |engine - reference| = {float(np.abs(logits[r][0] - z['logits'][r]).max()):.3g}")
    for r in (0, 1, 2):
        np.testing.assert_allclose(logits[r][0], z["logits"][r], rtol=0, atol=5e-5, err_msg=f"hidden {hidden} step {r}")


@pytest.mark.parametrize("preset", ["tiny-layer-a16", "tiny-hd80-a5"])
def test_adapter_kernels_are_what_run(preset):
    """One eager adapt call of one step (vanilla forward, backward, re-forward) with the census and timing on: no GEMM
    of the adapter's shapes is launched, the norm family counts exactly the adapter kernels more than the same
    geometry without adapters, and the workspace grows within the stated bound."""
    cfg, _ = model(preset)
    L, H, A = cfg["num_hidden_layers"], cfg["hidden_size"], cfg["adapter_attn_dim"]
    n = 32000
    T, B = num_frames(cfg, n), 2
    x = np.stack([synth.wave(n, 51), synth.wave(n, 52)])

    def census_of(e):
        e.set_graphs(False)
        e.set_timing(True)
        e.set_census(True)
        e.adapt(x, 1, SutaHParams(), record=[1])
        shapes = e.get_gemm_shape_times()
        norm = e.get_timing_ex()["norm"][1]
        e.set_census(False)
        e.set_timing(False)
        e.set_graphs(True)
        assert shapes
        nk = [tuple(int(re.search(rf"\b{c}=(\d+)", k).group(1)) for c in "NK") for k in shapes]
        return norm, [v for v in nk if v in ((A, H), (H, A))]

    norm_a, gemms = census_of(engine(preset))
    assert not gemms, gemms
    ws_a = engine(preset).workspace_bytes()
    norm_p, _ = census_of(engine(preset + "-plain"))
    ws_p = engine(preset + "-plain").workspace_bytes()
    # suta_adapt's minimal schedule: the vanilla forward (L adapter forwards), then per step one backward (L launches of
    # the backward: its tile-partial reduction is timed with it as one launch) and one forward (L): 2 L per step + L.
    # (The reference schedule's 3 L per step -- grad forward, backward, re-inference -- is what suta_step runs.)
    assert norm_a - norm_p == 2 * L * 1 + L, (norm_a, norm_p)
    bound = L * (4 * B * T * (H + A + 2) + 3 * 256)   # + the allocator's 256-B alignment of the three buffers
    assert 0 < ws_a - ws_p <= bound, (ws_a - ws_p, bound)


def test_step_schedule_counts_three_launches_per_layer():
    """suta_step (the reference schedule: grad forward, backward, re-inference) runs 3 L adapter launches per step."""
    cfg, _ = model("tiny-layer-a16")
    L = cfg["num_hidden_layers"]
    x = synth.wave(10960, 53)
    counts = []
    for key in ("tiny-layer-a16", "tiny-layer-a16-plain"):
        e = engine(key)
        e.reset()
        e.set_timing(True)
        e.step(x, SutaHParams())
        counts.append(e.get_timing_ex()["norm"][1])
        e.set_timing(False)
        e.reset()
    assert counts[0] - counts[1] == 3 * L, counts


def test_ragged_batch_equals_single_runs():
    """adapt_varlen of (32000, 19200) samples equals the two utterances alone: padding rows enter no statistic and no
    dgamma / dbeta, and each slot reads and adapts its own adapter LayerNorm."""
    eng = engine("tiny-layer-a16")
    cfg, sd = model("tiny-layer-a16")
    waves = [synth.wave(32000, 61), synth.wave(19200, 62)]
    hp = SutaHParams(lr=5e-4)
    steps = 3
    lv, iv, tv = eng.adapt_varlen(waves, steps, hp, record=[0, steps])
    names = adapter_norms(cfg)
    pv = [{n: eng.get_param(b, n) for n in names} for b in range(2)]
    for b, w in enumerate(waves):
        ls, _, T = eng.adapt(w, steps, hp, record=[0, steps])
        assert tv[b] == T
        for r in (0, steps):
            np.testing.assert_allclose(lv[r][b], ls[r][0], rtol=0, atol=2e-5, err_msg=f"utterance {b} step {r}")
        for n in names:
            assert_params_close(pv[b][n], eng.get_param(0, n), hp.lr, steps, name=n)
    for n in names:
        assert not np.array_equal(pv[0][n], pv[1][n]), f"slots did not diverge: {n}"
        assert not np.array_equal(pv[0][n], sd[n]), f"not adapted: {n}"


@pytest.mark.parametrize("key", ["tiny-layer-a16", "h1280"])
def test_bf16_mode_tracks_fp32(key):
    """bf16 GEMM mode (the adapter stays exact fp32 and hands its input gradient's bf16 plane to the FFN backward)."""
    eng = engine(key)
    x = synth.wave(32000, 63)
    ref, _, _ = eng.adapt(x, 3, SutaHParams(), record=[0, 3])
    eng.set_precision("bf16")
    try:
        got, ids, _ = eng.adapt(x, 3, SutaHParams(), record=[0, 3])
    finally:
        eng.set_precision("fp32")
    for r in (0, 3):
        assert np.isfinite(got[r]).all()
        assert_bf16_close(got[r][0], ref[r][0], 0.9, f"{key} step {r}")
        np.testing.assert_array_equal(ids[r][0], got[r][0].argmax(-1))


def test_deterministic_and_graph_replay_equals_eager():
    """Two identical calls are bitwise equal (tile partials summed in a fixed order, no float atomics), and the
    replayed hipGraph of the loop gives the eager call's ids and adapted tensors bitwise."""
    cfg, sd = model("tiny-layer-a16")
    eng = SutaEngine(cfg, sd, max_batch=2, max_samples=64000)
    names = eng.trainable_names()
    assert set(adapter_norms(cfg)) <= set(names)
    x = np.stack([synth.wave(32000, 71), synth.wave(32000, 72)])
    hp, rec = SutaHParams(), [0, 2]
    eng.adapt(x, 2, hp, record=rec, want_logits=False)
    assert eng.graph_stats()["last"] == "eager"
    eng.adapt(x, 2, hp, record=rec, want_logits=False)
    assert eng.graph_stats()["last"] == "captured"
    _, ids_r, _ = eng.adapt(x, 2, hp, record=rec, want_logits=False)
    assert eng.graph_stats()["last"] == "replayed"
    par_r = {b: {n: eng.get_param(b, n) for n in names} for b in range(2)}
    l1, ids1, _ = eng.adapt(x, 2, hp, record=rec)
    assert eng.graph_stats()["last"] == "eager"
    par_1 = {b: {n: eng.get_param(b, n) for n in names} for b in range(2)}
    eng.set_graphs(False)
    l2, ids2, _ = eng.adapt(x, 2, hp, record=rec)
    for r in rec:
        assert np.array_equal(l1[r], l2[r]), f"rerun differs at step {r}"
        assert np.array_equal(ids_r[r], ids1[r]), f"replayed ids != eager ids at step {r}"
    for b in range(2):
        for n in names:
            assert np.array_equal(par_1[b][n], eng.get_param(b, n)), f"rerun differs: slot {b} {n}"
            assert np.array_equal(par_r[b][n], par_1[b][n]), f"replayed != eager: slot {b} {n}"
    eng.close()


def test_refusals():
    cfg = get_config("tiny-layer-a16")
    cfg["adapter_attn_dim"] = 65
    with pytest.raises(RuntimeError, match=r"libsuta error 3: .*adapter_attn_dim > 64"):
        SutaEngine(cfg, synth_weights(cfg), max_batch=1, max_samples=32000)
    cfg, sd = model("tiny-layer-a16")
    name = "wav2vec2.encoder.layers.1.adapter_layer.linear_2.bias"
    with pytest.raises(RuntimeError, match=r"libsuta error 1: .*" + re.escape(name)):
        SutaEngine(cfg, {k: v for k, v in sd.items() if k != name}, max_batch=1, max_samples=32000)
    # the post-LN layer class builds no adapter: the field is ignored, the tensors are neither required nor read
    cfg = get_config("tiny-group")
    sd = synth_weights(cfg)
    x = synth.wave(8000, 81)
    a = SutaEngine(cfg, sd, max_batch=1, max_samples=32000)
    la = a.forward(x)
    a.close()
    b = SutaEngine(dict(cfg, adapter_attn_dim=16), sd, max_batch=1, max_samples=32000)
    assert np.array_equal(b.forward(x), la)
    b.close()


def test_cli_target_lang(tmp_path):
    """--asr <synthetic MMS directory> --target_lang xx: the driver overlays adapter.xx.safetensors (adapters and the
    language's 40-class lm_head) and decodes with xx's table of the nested vocab.json."""
    from safetensors.numpy import save_file
    from suta_amd.data import AudioReader, CHiMEDataset
    from suta_amd.decode import batch_decode, load_vocab, wer_counts
    from suta_amd.synth import normalize
    from suta_amd.weights import load_adapter, load_hf_checkpoint
    from tests import corpus_fixtures as CF
    from tests.multirank import run_ranks
    CF.chime(tmp_path, n=3)
    cfg = get_config("tiny-layer-a16")
    sd = synth_weights(cfg)
    lang_cfg = dict(cfg, vocab_size=40)
    lang_sd = synth_weights(lang_cfg, seed=7)
    ad = {k: v for k, v in lang_sd.items() if ".adapter_layer." in k or k.startswith("lm_head.")}
    letters = ["<pad>", "<s>", "</s>", "<unk>", "|"] + list("ETAONIHSRDLUWMCFGYPBVKXJQZ") + list("0123456789")[:9]
    vocab = {"xx": {t: i for i, t in enumerate(letters)}, "yy": {t: i for i, t in enumerate(reversed(letters[:32]))}}
    ck = tmp_path / "ckpt"
    ck.mkdir()
    json.dump(cfg, open(ck / "config.json", "w"))
    json.dump(vocab, open(ck / "vocab.json", "w"))
    save_file(sd, str(ck / "model.safetensors"))
    save_file(ad, str(ck / "adapter.xx.safetensors"))
    argv = (f"--asr {ck} --target_lang xx --steps 1 --dataset_name chime --dataset_dir {tmp_path} --episodic "
            f"--em_coef 0.3 --reweight --non_blank --train_feature --lr 5e-4 --log_dir {tmp_path}/exps --gpu_batch 1 "
            f"--device 0").split()
    (counts,), (out,) = run_ranks(1, argv, tmp_path, fake=False)
    # the same through the library: overlay, adapt, decode with xx's table
    c2, s2 = get_config(str(ck)), load_hf_checkpoint(str(ck))
    load_adapter(str(ck), "xx", c2, s2)
    assert c2["vocab_size"] == 40
    eng = SutaEngine(c2, s2, max_batch=1, max_samples=64000)
    vx = load_vocab(str(ck), target_lang="xx")
    ds = CHiMEDataset(None, 1, str(tmp_path))
    reader = AudioReader(0.0)
    hyps = {0: [], 1: []}
    hp = SutaHParams(lr=5e-4, em_coef=0.3)
    for f in ds.file_list:
        _, ids, _ = eng.adapt(normalize(reader(str(f))), 1, hp, record=[0, 1], want_logits=False)
        for r in hyps:
            hyps[r].append(batch_decode(ids[r], vocab=vx)[0])
    eng.close()
    assert out.count("original WER: ") >= len(ds.file_list)
    for r in hyps:
        assert tuple(counts[str(r)]) == wer_counts(list(ds.text), hyps[r]), r
