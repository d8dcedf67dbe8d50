"""GPU tier: HuBERT and data2vec-audio CTC checkpoints -- the state-dict prefix by `model_family`, and data2vec's
positional stack (per layer: the grouped conv on posconv_kernel's epilogue-free form or the conv-A GEMM, then the fused
LayerNorm(no affine) -> GELU row kernels of csrc/ops.hip), forward and backward.

The reference is the reference's own forward_and_adapt on HF's Data2VecAudioForCTC / HubertForCTC, recorded by
tests/golden/make_golden_families.py (g16_*); every fixture's `posconv_effect` (step-0 logits with the positional
embedding forced to zero) is more than 100 x the tolerance applied here, so a run that skipped it cannot pass.  The tiny
fixtures' waveforms are those on which the reference's own fp32 run stays within half of logits_tol of its float64 run
(`ref_f32_err`; tests/test_gpu_adapter.py explains why).

Tolerances are the project's own for each comparison:
  * tiny models against the reference: tests/parity.logits_tol(lr); adapted tensors by tests/parity.assert_params_close,
    the Adam budget from the tensor's multiplicity in the fixture's own `entries`
  * full-width models: atol 5e-5 on logits (tests/test_gpu_adapter.py's full-width bound)
  * a ragged batch against the single runs: tests/test_gpu_varlen.py's equality
  * bf16 mode against exact fp32: tests/parity.assert_bf16_close
  * the wav2vec2 positional conv against the parent commit's recording, graph against eager: bitwise
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
from suta_amd.modules import collect_params
from suta_amd.weights import synth_weights
from tests.parity import adam_multiplicity, assert_bf16_close, assert_params_close, logits_tol

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def wide_cfg(hidden):
    """tests/test_gpu_headdim.py::wide_cfg as data2vec-audio (make_golden_families.wide_cfg): one layer at full width,
    16 positional-conv groups of width hidden / 16, depth 5, k 19."""
    cfg = get_config("data2vec-audio-base")
    cfg.update(hidden_size=hidden, num_attention_heads=16, num_conv_pos_embedding_groups=16, num_hidden_layers=1,
               intermediate_size=256, conv_dim=[32] * 7)
    return cfg


def w2v2_wide_cfg(hidden):
    """tests/test_gpu_headdim.py::wide_cfg itself (wav2vec2, one K = 128 weight-normed positional conv)."""
    cfg = get_config("wav2vec2-xls-r-1b")
    cfg.update(hidden_size=hidden, num_attention_heads=16, num_conv_pos_embedding_groups=16, num_hidden_layers=1,
               intermediate_size=256, conv_dim=[32] * 7)
    return cfg


def model(key):
    if ("model", key) not in _CACHE:
        cfg = wide_cfg(int(key[1:])) if key.startswith("h") else w2v2_wide_cfg(int(key[5:])) \
            if key.startswith("w2v2h") else get_config(key)
        _CACHE[("model", key)] = (cfg, synth_weights(cfg))
    return _CACHE[("model", key)]


def engine(key):
    if ("engine", key) not in _CACHE:
        cfg, sd = model(key)
        _CACHE[("engine", key)] = SutaEngine(cfg, sd, max_batch=3, max_samples=64000)
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


def params_close(got, want, lr, steps, name, entries):
    """assert_params_close with the Adam budget k * steps * lr, k the tensor's count in the fixture's collect_params
    entries (parity.adam_multiplicity knows `wav2vec2.` names only and answers 5 for these)."""
    k = sum(1 for e in entries if e == name)
    assert k >= 1, name
    assert_params_close(got, want, lr, steps, name=name, factor=k / adam_multiplicity(name))


TINY_FIXTURES = [("tiny-d2v", "g16_d2v_tiny_N400.npz"), ("tiny-d2v", "g16_d2v_tiny_N10960.npz"),
                 ("tiny-d2v", "g16_d2v_tiny_N32000.npz"), ("tiny-d2v", "g16_d2v_tiny_N10960_biasonly.npz"),
                 ("tiny-d2v-even", "g16_d2v_even_N10960.npz"), ("tiny-hubert", "g16_hubert_tiny_N10960.npz")]


def _fixture(preset, fname):
    z = np.load(os.path.join(G, fname))
    cfg, sd = model(preset)
    assert digest(sd) == str(z["weights_sha256"]), "seeded weight generator drifted"
    h = ast.literal_eval(str(z["hp_json"]))
    tol = logits_tol(h["lr"])
    assert float(z["posconv_effect"]) > 100 * tol
    assert float(z["ref_f32_err"].max()) <= 0.5 * tol
    return z, h, tol


@pytest.mark.parametrize("preset,fname", TINY_FIXTURES)
def test_tiny_matches_reference(preset, fname):
    """4 SUTA steps at lr 5e-4 on HF's model (T = 1, 34, 99: 34 frames are fewer than the stack's 91-frame receptive
    field; --bias_only; the even kernel size 4, where HF trims a frame; HuBERT): logits of every step, the adapted
    tensors, greedy ids."""
    z, h, tol = _fixture(preset, fname)
    steps = int(z["steps"])
    eng = engine(preset)
    hp = SutaHParams(lr=h["lr"], temp=h["temp"], em_coef=h["em"], reweight=h["rw"], non_blank=h["nb"],
                     div_coef=h["div"], train_feature=h["train_feature"], bias_only=h["bias_only"])
    logits, ids, T = eng.adapt(z["x"], steps, hp, record=list(range(steps + 1)))
    ref = z["logits"]
    assert T == ref.shape[1]
    for i in range(steps + 1):
        print(f"{fname} step {i}: max |engine - reference| = {float(np.abs(logits[i][0] - ref[i]).max()):.3g}")
    for i in range(steps + 1):
        np.testing.assert_allclose(logits[i][0], ref[i], rtol=0, atol=tol, err_msg=f"{fname} step {i}")
        np.testing.assert_array_equal(ids[i][0], logits[i][0].argmax(-1))
    entries = [str(e) for e in z["entries"]]
    finals = [k[len("final/"):] for k in z.files if k.startswith("final/")]
    assert set(finals) == set(entries) and finals
    assert all(n.startswith(("hubert." if preset == "tiny-hubert" else "data2vec_audio.")) for n in finals)
    for name in finals:
        params_close(eng.get_param(0, name), z["final/" + name], h["lr"], steps, name, entries)
    assert sorted(eng.trainable_names()) == sorted(set(collect_params(model(preset)[0], False, True)[1]))


def _wide_run(eng, hidden):
    z = np.load(os.path.join(G, f"g16_d2v_h{hidden}_N48000.npz"))
    assert digest(model(f"h{hidden}")[1]) == str(z["weights_sha256"]), "seeded weight generator drifted"
    assert float(z["posconv_effect"]) > 100 * 5e-5
    n, seed = (int(v) for v in z["wave"])
    logits, ids, T = eng.adapt(synth.wave(n, seed), 2, SutaHParams(), record=[0, 1, 2])
    assert T == 149 == z["logits"].shape[1]   # two frame tiles of the kernel, the second with tail rows
    return logits, z["logits"]


@pytest.mark.parametrize("hidden", [768, 1024])
def test_full_width_matches_reference_on_kernel_path(hidden):
    """Group widths 48 / 64: the stack's convs on posconv_kernel (zero-filled 20th tap), 2 steps."""
    logits, ref = _wide_run(engine(f"h{hidden}"), hidden)
    for r in (0, 1, 2):
        print(f"hidden {hidden} step {r}: max |engine - reference| = {float(np.abs(logits[r][0] - ref[r]).max()):.3g}")
    for r in (0, 1, 2):
        np.testing.assert_allclose(logits[r][0], ref[r], rtol=0, atol=5e-5, err_msg=f"hidden {hidden} step {r}")


@pytest.mark.parametrize("hidden", [768, 1024])
def test_full_width_matches_reference_on_gemm_path(hidden, monkeypatch):
    """SUTA_POSCONV=0: the same convs as conv-A GEMMs, against the golden (not against the kernel path)."""
    monkeypatch.setenv("SUTA_POSCONV", "0")
    cfg, sd = model(f"h{hidden}")
    eng = SutaEngine(cfg, sd, max_batch=1, max_samples=64000)
    try:
        logits, ref = _wide_run(eng, hidden)
    finally:
        eng.close()
    for r in (0, 1, 2):
        print(f"hidden {hidden} GEMM path step {r}: max |engine - reference| = "
              f"{float(np.abs(logits[r][0] - ref[r]).max()):.3g}")
    for r in (0, 1, 2):
        np.testing.assert_allclose(logits[r][0], ref[r], rtol=0, atol=5e-5, err_msg=f"hidden {hidden} step {r}")


def test_stack_kernels_are_what_run(monkeypatch):
    """One eager step with the census and timing on at H = 768: on the default path no GEMM of the stack's shape
    (N = 48, K = 19 * 48) is launched; under SUTA_POSCONV=0 there are 5 per forward and 5 per backward.  The row
    kernels count into the norm family: 5 per forward and 5 per backward more than the norm launches of the same
    geometry as wav2vec2 (whose positional conv has none)."""
    cfg, sd = model("h768")
    x = synth.wave(48000, 7)

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
        nk = {k: v[0] for k, v in shapes.items()
              if tuple(int(re.search(rf"\b{c}=(\d+)", k).group(1)) for c in "NK") == (48, 19 * 48)}
        return norm, sum(nk.values())

    norm_k, gemms_k = census_of(engine("h768"))
    assert gemms_k == 0
    monkeypatch.setenv("SUTA_POSCONV", "0")
    eng = SutaEngine(cfg, sd, max_batch=1, max_samples=64000)
    try:
        norm_g, gemms_g = census_of(eng)
    finally:
        eng.close()
    # suta_adapt's minimal schedule for one step: vanilla forward, backward, forward
    assert gemms_g == 5 * 3 and norm_g == norm_k
    # the same geometry as post-LN wav2vec2 with the layer-norm front end: every other norm launch is the same
    wcfg = dict(cfg, num_conv_pos_embeddings=128)
    for k in ("model_type", "conv_pos_kernel_size"):
        wcfg.pop(k)
    w = SutaEngine(wcfg, synth_weights(wcfg), max_batch=1, max_samples=64000)
    try:
        norm_w, _ = census_of(w)
    finally:
        w.close()
    assert norm_k - norm_w == 5 * 3, (norm_k, norm_w)


def test_wav2vec2_positional_conv_is_bitwise_the_parent_commits():
    """tiny-layer (the conv-A GEMM) and the one-layer H = 768 wav2vec2 model (posconv_kernel, K = 128) give bitwise
    the logits recorded on the commit before the stack's epilogues were compiled into the kernel."""
    z = np.load(os.path.join(G, "g16_w2v2_posconv_parent.npz"))
    for key in ("tiny-layer", "w2v2h768"):
        cfg, sd = model(key)
        assert digest(sd) == str(z[f"{key}/weights_sha256"]), "seeded weight generator drifted"
        n, seed = (int(v) for v in z[f"{key}/wave"])
        eng = SutaEngine(cfg, sd, max_batch=1, max_samples=64000)
        try:
            logits, _, _ = eng.adapt(synth.wave(n, seed), 2, SutaHParams(), record=[0, 1, 2])
        finally:
            eng.close()
        for r in (0, 1, 2):
            assert np.array_equal(logits[r][0], z[f"{key}/logits"][r]), f"{key} step {r}"


def _check_against_singles(eng, waves, steps, hp, record):
    """tests/test_gpu_varlen.py::_check_against_singles."""
    lv, iv, tv = eng.adapt_varlen(waves, steps, hp, record=record)
    finals = [{n: eng.get_param(b, n) for n in eng.trainable_names()} for b in range(len(waves))]
    entries = collect_params(eng.cfg, hp.bias_only, hp.train_feature)[1]
    for b, w in enumerate(waves):
        l1, i1, t1 = eng.adapt(w, steps, hp, record=record)
        assert tv[b] == t1
        for r in record:
            print(f"utt {b} step {r}: max |ragged - alone| = {float(np.abs(lv[r][b] - l1[r][0]).max()):.3g}")
            np.testing.assert_allclose(lv[r][b], l1[r][0], rtol=0, atol=logits_tol(hp.lr), err_msg=f"utt {b} step {r}")
            assert np.mean(iv[r][b] == i1[r][0]) > 0.99
        for n in eng.trainable_names():
            params_close(finals[b][n], eng.get_param(0, n), hp.lr, steps, n, entries)


def test_ragged_batch_equals_single_runs_tiny():
    """(32000, 10960, 400) samples = (99, 34, 1) frames, the fixtures' waveforms: a padded frame is 0 after the row
    kernel and the next conv would add its bias there, so every layer's window must read it as zero."""
    waves = [np.load(os.path.join(G, f"g16_d2v_tiny_N{n}.npz"))["x"] for n in (32000, 10960, 400)]
    _check_against_singles(engine("tiny-d2v"), waves, 3, SutaHParams(lr=5e-4), [0, 1, 3])


def test_ragged_batch_equals_single_runs_full_width():
    """(48000, 20000) samples = (149, 62) frames at H = 768 on the kernel path: the short utterance ends inside the
    first frame tile."""
    waves = [synth.wave(48000, 91), synth.wave(20000, 92)]
    _check_against_singles(engine("h768"), waves, 2, SutaHParams(), [0, 2])


def test_graph_replay_equals_eager():
    cfg, sd = model("tiny-d2v")
    eng = SutaEngine(cfg, sd, max_batch=2, max_samples=64000)
    names = eng.trainable_names()
    x = np.stack([synth.wave(32000, 71), synth.wave(32000, 72)])
    hp, rec = SutaHParams(lr=5e-4), [0, 2]
    eng.adapt(x, 2, hp, record=rec, want_logits=False)
    eng.adapt(x, 2, hp, record=rec, want_logits=False)
    assert eng.graph_stats()["last"] == "captured"
    _, ids_r, _ = eng.adapt(x, 2, hp, record=rec, want_logits=False)
    assert eng.graph_stats()["last"] == "replayed"
    par_r = {b: {n: eng.get_param(b, n) for n in names} for b in range(2)}
    eng.set_graphs(False)
    l2, ids2, _ = eng.adapt(x, 2, hp, record=rec)
    assert eng.graph_stats()["last"] == "eager"
    for r in rec:
        assert np.array_equal(ids_r[r], ids2[r]), f"replayed ids != eager ids at step {r}"
    for b in range(2):
        for n in names:
            assert np.array_equal(par_r[b][n], eng.get_param(b, n)), f"replayed != eager: slot {b} {n}"
            assert not np.array_equal(par_r[b][n], sd[n]), f"not adapted: {n}"
    eng.close()


def test_bf16_mode_tracks_fp32():
    """bf16 GEMM mode: the stack's convs on the mode's conv-A GEMM, LayerNorm and GELU in fp32."""
    eng = engine("tiny-d2v")
    x = synth.wave(32000, 63)
    ref, _, _ = eng.adapt(x, 3, SutaHParams(), record=[0, 3])
    eng.set_precision("bf16")
    try:
        got, ids, _ = eng.adapt(x, 3, SutaHParams(), record=[0, 3])
    finally:
        eng.set_precision("fp32")
    for r in (0, 3):
        assert np.isfinite(got[r]).all()
        assert_bf16_close(got[r][0], ref[r][0], 0.9, f"tiny-d2v step {r}")
        np.testing.assert_array_equal(ids[r][0], got[r][0].argmax(-1))


def test_reference_loop_through_shim():
    """The reference loop of suta.py's docstring with the shim's objects on tiny-d2v reproduces g16_d2v_tiny_N10960."""
    import contextlib
    import io
    import torch
    from suta_amd import suta as S
    z, h, tol = _fixture("tiny-d2v", "g16_d2v_tiny_N10960.npz")
    cfg, sd = model("tiny-d2v")
    m = S.configure_model(S.Wav2Vec2ForCTC(cfg, sd).eval().cuda())
    with contextlib.redirect_stdout(io.StringIO()) as out:
        params, names = S.collect_params(m, h["bias_only"], h["train_feature"], False, True)
        optimizer, scheduler = S.setup_optimizer(params, "AdamW", h["lr"], scheduler=None)
    assert list(names) == [str(e) for e in z["entries"]]
    assert "data2vec_audio.encoder.pos_conv_embed.layers.0.conv" in out.getvalue().split("\n")
    states = S.copy_model_and_optimizer(m, optimizer, scheduler)
    m, optimizer, scheduler = S.load_model_and_optimizer(m, optimizer, *states)
    x = torch.from_numpy(z["x"])[None]
    with torch.no_grad():
        outputs = m(x).logits
    np.testing.assert_allclose(outputs[0].cpu().numpy(), z["logits"][0], rtol=0, atol=tol)
    for i in range(int(z["steps"])):
        outputs = S.forward_and_adapt(x, m, optimizer, h["em"], h["rw"], h["temp"], h["nb"], scheduler, h["div"])
        np.testing.assert_allclose(outputs[0].cpu().numpy(), z["logits"][i + 1], rtol=0, atol=tol, err_msg=f"step {i + 1}")
    sdf = m.state_dict()
    entries = [str(e) for e in z["entries"]]
    for name in dict.fromkeys(entries):
        params_close(sdf[name].numpy(), z["final/" + name], h["lr"], int(z["steps"]), name, entries)
    m.close()


def test_refusals():
    cfg, sd = model("tiny-d2v")
    with pytest.raises(RuntimeError, match=r"libsuta error 1: .*do_stable_layer_norm"):
        SutaEngine(dict(cfg, do_stable_layer_norm=True), sd, max_batch=1, max_samples=32000)
    with pytest.raises(RuntimeError, match=r"libsuta error 1: .*feat_extract_norm_layer"):
        SutaEngine(dict(cfg, feat_extract_norm="group"), sd, max_batch=1, max_samples=32000)
    deep = dict(cfg, num_conv_pos_embeddings=9)
    with pytest.raises(RuntimeError, match=r"libsuta error 3: .*num_conv_pos_embeddings"):
        SutaEngine(deep, synth_weights(deep), max_batch=1, max_samples=32000)
    long = dict(cfg, conv_pos_kernel_size=129)
    with pytest.raises(RuntimeError, match=r"libsuta error 3: .*conv_pos_kernel_size"):
        SutaEngine(long, synth_weights(long), max_batch=1, max_samples=32000)
    name = "data2vec_audio.encoder.pos_conv_embed.layers.3.conv.bias"
    with pytest.raises(RuntimeError, match=r"libsuta error 1: .*" + re.escape(name)):
        SutaEngine(cfg, {k: v for k, v in sd.items() if k != name}, max_batch=1, max_samples=32000)
    # a wav2vec2 state dict under a HuBERT config: the required names carry the family's prefix
    hcfg, hsd = model("tiny-hubert")
    wsd = {k.replace("hubert.", "wav2vec2.", 1): v for k, v in hsd.items()}
    with pytest.raises(RuntimeError, match=r"libsuta error 1: missing weight hubert\."):
        SutaEngine(hcfg, {**wsd, **{k: hsd[k] for k in ("lm_head.weight", "lm_head.bias")}}, max_batch=1,
                   max_samples=32000)


def test_cli_runs_a_data2vec_checkpoint_directory(tmp_path):
    """main.py --asr <directory with config.json (model_type data2vec-audio) + model.safetensors>: runs end to end and
    prints the reference's parameter names under the `data2vec_audio.` prefix."""
    from safetensors.numpy import save_file
    from tests import corpus_fixtures as CF
    from tests.multirank import run_ranks
    CF.chime(tmp_path, n=3)
    cfg, sd = model("tiny-d2v")
    ck = tmp_path / "ckpt"
    ck.mkdir()
    hf = {k: v for k, v in cfg.items() if k not in ("feat_extract_norm", "do_stable_layer_norm")}   # HF has neither
    json.dump(hf, open(ck / "config.json", "w"))
    save_file(sd, str(ck / "model.safetensors"))
    assert get_config(str(ck)) == cfg
    argv = (f"--asr {ck} --steps 1 --dataset_name chime --dataset_dir {tmp_path} --episodic --em_coef 0.3 --reweight "
            f"--non_blank --train_feature --lr 5e-4 --log_dir {tmp_path}/exps --gpu_batch 1 --device 0").split()
    (counts,), (out,) = run_ranks(1, argv, tmp_path, fake=False)
    printed, names = collect_params(cfg, False, True)
    assert str(names) in out.split("\n")
    assert all(n.startswith("data2vec_audio.") for n in names)
    lines = out.split("\n")
    assert "data2vec_audio.encoder.pos_conv_embed.layers.4.layer_norm" in lines
    assert out.count("original WER: ") >= 3
    assert {"0", "1"} <= set(counts)   # WER counts of the unadapted and the one-step hypotheses
