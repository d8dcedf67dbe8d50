"""Golden vectors for the HuBERT and data2vec-audio families, from the REFERENCE's own code on HF's models.

Build container only (it reads the reference checkout through make_golden.py, whose helpers it imports):
    python tests/golden/make_golden_families.py

  g16_family_keys.json    HF `Data2VecAudioForCTC` / `HubertForCTC` `state_dict()` keys of tiny-d2v and tiny-hubert, and
                          the reference's collect_params names and printed module names for (bias_only, train_feature) =
                          (False, True), (True, True), (False, False).
  g16_d2v_tiny_N{400,10960,32000}.npz (T = 1, 34, 99; 34 frames are fewer than the stack's 91-frame receptive field),
  g16_d2v_tiny_N10960_biasonly.npz, g16_d2v_even_N10960.npz (tiny-d2v-even: k = 4, HF trims the last frame),
  g16_hubert_tiny_N10960.npz
                          episodic SUTA (main.py:327-348), 4 steps, lr 5e-4, the scripts' flags: logits after every
                          step + final trainable tensors (g11's layout).
  g16_d2v_h{768,1024}_N48000.npz
                          the one-layer full-width model of tests/test_gpu_headdim.py::wide_cfg as data2vec-audio (16
                          groups of width 48 / 64, depth 5, k 19), T = 149: 2 steps at the default hparams, logits of
                          steps 0..2, the weights' digest.

(g16_w2v2_posconv_parent.npz is no output of this script: tests/golden/record_posconv_baseline.py records it on the GPU.)

Every fixture carries `posconv_effect`: max |step-0 logits - the same model's with the positional embedding forced to
zero|.  The script asserts it above 100 x the tolerance the GPU test applies (tests/parity.logits_tol(lr) on the tiny
models, 5e-5 at full width), so a run that skipped the positional embedding cannot pass.  The tiny fixtures also carry
`ref_f32_err`: per step, max |the reference's fp32 logits - its own float64 run's|, at most half of logits_tol(lr) by
the choice of the waveform (make_golden_adapter.tiny explains why).
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

from suta_amd.config import family, get_config  # noqa: E402
from suta_amd.weights import synth_weights  # noqa: E402

sys.path.insert(0, mg.REPO)
from tests.parity import logits_tol  # noqa: E402


def hf_model(cfg, sd=None):
    from transformers import Data2VecAudioConfig, Data2VecAudioForCTC, HubertConfig, HubertForCTC
    kw = {k: v for k, v in cfg.items() if k != "model_type"}
    torch.manual_seed(0)
    if family(cfg) == "data2vec-audio":
        m = Data2VecAudioForCTC(Data2VecAudioConfig(**kw)).eval()
    else:
        assert family(cfg) == "hubert"
        m = HubertForCTC(HubertConfig(**kw)).eval()
    if sd is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def keys(ref):
    out = {}
    for preset in ("tiny-d2v", "tiny-hubert"):
        m = hf_model(get_config(preset))
        ent = {"state_dict": list(m.state_dict().keys())}
        for bias_only, train_feature in ((False, True), (True, True), (False, False)):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                _, names = ref.collect_params(m, bias_only, train_feature, False, True)
            ent[f"bias_only={bias_only},train_feature={train_feature}"] = list(names)
            ent["printed"] = buf.getvalue().split("\n")[:-1]   # one module name per line (the root's is empty)
        out[preset] = ent
    with open(os.path.join(HERE, "g16_family_keys.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("keys done")


def run_ref(ref, cfg, sd, x, steps, lr, train_feature=True, bias_only=False, em=0.3, rw=True, nb=True, temp=2.5,
            div=0.0, double=False):
    """make_golden.run_ref_suta on the family's HF model; double: model, waveform and optimizer state in float64."""
    model = hf_model(cfg, sd)
    model = ref.configure_model(model.double() if double else model)
    with contextlib.redirect_stdout(io.StringIO()):
        params, names = ref.collect_params(model, bias_only, train_feature, False, True)
        opt, sch = ref.setup_optimizer(params, "AdamW", lr, scheduler=None)
    xt = torch.from_numpy(x)[None]
    xt = xt.double() if double else xt
    with torch.no_grad():
        logits = [model(xt).logits[0].numpy().copy()]
    for _ in range(steps):
        logits.append(ref.forward_and_adapt(xt, model, opt, em, rw, temp, nb, sch, div)[0].detach().numpy().copy())
    sdf = model.state_dict()
    return np.stack(logits), {n: sdf[n].numpy().copy() for n in dict.fromkeys(names)}, names


def posconv_effect(cfg, sd, x, logits0):
    m = hf_model(cfg, sd)
    base = getattr(m, "data2vec_audio" if family(cfg) == "data2vec-audio" else "hubert")
    base.encoder.pos_conv_embed.register_forward_hook(lambda mod, inp, out: torch.zeros_like(out))
    with torch.no_grad():
        l0 = m(torch.from_numpy(x)[None]).logits[0].numpy()
    return float(np.abs(l0 - logits0).max())


def tiny(ref, only=None):
    steps, lr = 4, 5e-4
    runs = [("d2v_tiny", "tiny-d2v", 400, False), ("d2v_tiny", "tiny-d2v", 10960, False),
            ("d2v_tiny", "tiny-d2v", 32000, False), ("d2v_tiny", "tiny-d2v", 10960, True),
            ("d2v_even", "tiny-d2v-even", 10960, False), ("hubert_tiny", "tiny-hubert", 10960, False)]
    for j, (tag, preset, n, bias_only) in enumerate(runs):
        if only and tag != only:
            continue
        cfg = get_config(preset)
        sd = synth_weights(cfg)
        hp = dict(lr=lr, train_feature=True, bias_only=bias_only, em=0.3, rw=True, nb=True, temp=2.5, div=0.0)
        seed = 170 + j

        def attempt():
            x = mg.wave(n, seed)
            logits, final, names = run_ref(ref, cfg, sd, x, steps, **hp)
            l64, _, _ = run_ref(ref, cfg, sd, x, steps, double=True, **hp)
            return x, logits, final, names, np.abs(l64 - logits).reshape(steps + 1, -1).max(1)
        x, logits, final, names, ref_err = attempt()
        # make_golden_adapter.tiny: at T = 1 a blank frame leaves the gradient pure rounding noise, and at any T a
        # waveform on which the reference's own fp32 run is off by more than half the bound cannot test at that bound
        while (logits[0].shape[0] == 1 and any(int(logits[i].argmax(-1)[0]) == 0 for i in range(steps + 1))) or \
                ref_err.max() > 0.5 * logits_tol(lr):
            print("  skip seed", seed, "ref fp32-vs-fp64", ref_err)
            seed += 100
            x, logits, final, names, ref_err = attempt()
        eff = posconv_effect(cfg, sd, x, logits[0])
        assert eff > 100 * logits_tol(lr), (tag, n, eff)
        out = {"weights_sha256": np.array(mg.weights_digest(sd)), "hp_json": np.array(repr(hp)),
               "steps": np.array(steps), "x": x, "logits": logits, "entries": np.array(names),
               "posconv_effect": np.array(eff), "wave_seed": np.array(seed), "ref_f32_err": ref_err}
        for k, v in final.items():
            out[f"final/{k}"] = v
        fn = f"g16_{tag}_N{n}{'_biasonly' if bias_only else ''}.npz"
        np.savez_compressed(os.path.join(HERE, fn), **out)
        print(fn, "T =", logits[0].shape[0], "seed", seed, "posconv_effect", eff, "ref fp32-vs-fp64", ref_err.max(),
              os.path.getsize(os.path.join(HERE, fn)))


def wide_cfg(hidden):
    """tests/test_gpu_headdim.py::wide_cfg as data2vec-audio: 16 positional-conv groups (width hidden / 16)."""
    cfg = get_config("data2vec-audio-base")
    cfg.update(hidden_size=hidden, num_attention_heads=16, num_conv_pos_embedding_groups=16, num_hidden_layers=1,
               intermediate_size=256, conv_dim=[32] * 7)
    return cfg


def wide(ref):
    for hidden in (768, 1024):
        cfg = wide_cfg(hidden)
        sd = synth_weights(cfg)
        seed = 180
        x = mg.wave(48000, seed)
        logits, _, _ = run_ref(ref, cfg, sd, x, 2, lr=2e-5)
        assert logits.shape[1] == 149
        eff = posconv_effect(cfg, sd, x, logits[0])
        assert eff > 100 * 5e-5, (hidden, eff)
        fn = f"g16_d2v_h{hidden}_N48000.npz"
        np.savez_compressed(os.path.join(HERE, fn), weights_sha256=np.array(mg.weights_digest(sd)),
                            wave=np.array([48000, seed]), logits=logits, posconv_effect=np.array(eff))
        print(fn, "posconv_effect", eff, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref = mg.import_reference()
    for w in sys.argv[1:] or ["keys", "tiny", "wide"]:
        if w.startswith("tiny:"):   # one tiny fixture by tag, e.g. tiny:d2v_even
            tiny(ref, only=w[5:])
        else:
            globals()[w](ref)
