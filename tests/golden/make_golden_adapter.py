"""Golden vectors for MMS attention adapters (`adapter_attn_dim`), from the REFERENCE's own code on HF's model.

Build container only (it reads the reference checkout through make_golden.py, whose helpers it imports):
    python tests/golden/make_golden_adapter.py

  g15_adapter_keys.json   HF `Wav2Vec2ForCTC.state_dict()` keys of tiny-layer-a16 and the reference's
                          collect_params names for (bias_only, train_feature) = (False, True), (True, True),
                          (False, False); the same for tiny-group with adapter_attn_dim=16 (HF's post-LN layer
                          builds no adapter: no adapter keys).
  g15_adapter_tiny_layer_a16_N{400,10960,32000}.npz, g15_adapter_tiny_hd80_a5_N10960.npz (T = 1, 34, 99),
  g15_adapter_tiny_h72_a16_N10960.npz (tiny-layer-a16 at hidden 72, no multiple of 16)
                          episodic SUTA (main.py:327-348), 4 steps, lr 5e-4, the scripts' flags: logits after every
                          step + final trainable tensors (g11's layout); ..._N10960_biasonly.npz: --bias_only.
  g15_adapter_h{1024,1280,2048}_a16_N32000.npz
                          the one-layer full-width model of tests/test_gpu_headdim.py::wide_cfg (16 heads) with the
                          adapter: 2 steps at the default hparams, logits of steps 0..2, the weights' digest.

Every fixture carries `adapter_effect`: max |step-0 logits - the same model's with linear_2 zeroed| (the adapter's
output removed).  The script asserts it above 100 x the tolerance the GPU test applies (tests/parity.logits_tol(lr) on
the tiny models, 5e-5 at full width), so a run that skipped the adapter cannot pass.  The tiny fixtures also carry
`ref_f32_err`: per step, max |the reference's fp32 logits - its own float64 run's|, at most half of logits_tol(lr) by
the choice of the waveform (see tiny()).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

from suta_amd.config import get_config  # noqa: E402
from suta_amd.weights import synth_weights  # noqa: E402

sys.path.insert(0, mg.REPO)
from tests.parity import logits_tol  # noqa: E402


def hf_model(cfg, sd=None):
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
    torch.manual_seed(0)
    m = Wav2Vec2ForCTC(Wav2Vec2Config(**cfg)).eval()
    if sd is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def keys(ref):
    import contextlib
    import io
    out = {}
    for tag, preset in (("tiny-layer-a16", "tiny-layer-a16"), ("tiny-group+a16", "tiny-group")):
        cfg = get_config(preset)
        cfg["adapter_attn_dim"] = 16
        m = hf_model(cfg)
        ent = {"state_dict": list(m.state_dict().keys())}
        for bias_only, train_feature in ((False, True), (True, True), (False, False)):
            with contextlib.redirect_stdout(io.StringIO()):
                _, names = ref.collect_params(m, bias_only, train_feature, False, True)
            ent[f"bias_only={bias_only},train_feature={train_feature}"] = list(names)
        out[tag] = ent
    with open(os.path.join(HERE, "g15_adapter_keys.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("keys done")


def adapter_effect(cfg, sd, x, logits0):
    off = {k: (np.zeros_like(v) if ".adapter_layer.linear_2." in k else v) for k, v in sd.items()}
    with torch.no_grad():
        l0 = hf_model(cfg, off)(torch.from_numpy(x)[None]).logits[0].numpy()
    return float(np.abs(l0 - logits0).max())


def run_ref_suta_f64(ref, cfg, sd, x, steps, lr, train_feature=True, bias_only=False, em=0.3, rw=True, nb=True,
                     temp=2.5, div=0.0):
    """make_golden.run_ref_suta with the model, the waveform and the optimizer state in float64: the logits of every
    step, against which the reference's own fp32 rounding error is measured."""
    import contextlib
    import io
    model = ref.configure_model(hf_model(cfg, sd).double())
    with contextlib.redirect_stdout(io.StringIO()):
        params, _ = ref.collect_params(model, bias_only, train_feature, False, True)
        opt, sch = ref.setup_optimizer(params, "AdamW", lr, scheduler=None)
    xt = torch.from_numpy(x).double()[None]
    with torch.no_grad():
        out = [model(xt).logits[0].numpy().copy()]
    for _ in range(steps):
        out.append(ref.forward_and_adapt(xt, model, opt, em, rw, temp, nb, sch, div)[0].detach().numpy().copy())
    return np.stack(out)


def h72_cfg():
    """hidden 72: a multiple of 8 that is no multiple of the adapter kernels' 16-column chunk (the last chunk is half
    empty); 4 heads of 18, 3 positional-conv groups of width 24."""
    cfg = get_config("tiny-layer-a16")
    cfg.update(hidden_size=72, num_attention_heads=4, num_conv_pos_embedding_groups=3)
    return cfg


def tiny(ref, only=None):
    steps, lr = 4, 5e-4
    runs = [("tiny_layer_a16", "tiny-layer-a16", 400, False), ("tiny_layer_a16", "tiny-layer-a16", 10960, False),
            ("tiny_layer_a16", "tiny-layer-a16", 32000, False), ("tiny_hd80_a5", "tiny-hd80-a5", 10960, False),
            ("tiny_layer_a16", "tiny-layer-a16", 10960, True), ("tiny_h72_a16", None, 10960, False)]
    for j, (tag, preset, n, bias_only) in enumerate(runs):
        if only and tag != only:
            continue
        cfg = get_config(preset) if preset else h72_cfg()
        sd = synth_weights(cfg)
        hp = dict(lr=lr, train_feature=True, bias_only=bias_only, em=0.3, rw=True, nb=True, temp=2.5, div=0.0)
        seed = 150 + j

        def attempt():
            x = mg.wave(n, seed)
            logits, final, names = mg.run_ref_suta(ref, cfg, sd, x, steps, **hp)
            l32 = np.stack([logits[i] for i in range(steps + 1)])
            err = np.abs(run_ref_suta_f64(ref, cfg, sd, x, steps, **hp) - l32).reshape(steps + 1, -1).max(1)
            return x, logits, final, names, err
        x, logits, final, names, ref_err = attempt()
        # T = 1: the MCC term of a single frame is the constant (V - 1) / 32 (the normalised covariance's rows are the
        # frame's softmax), and a blank frame leaves the non-blank entropy term empty, so the whole gradient is zero in
        # exact arithmetic and Adam steps on fp32 rounding noise alone: no two implementations agree there.  Take the
        # first seed whose frame stays non-blank through every step (the entropy term then gives a real gradient).
        #
        # Any T: Adam steps an element by lr g / (|g| + eps), so an element whose gradient is of the size of eps = 1e-8
        # is moved by a rounding-dependent fraction of lr, and the reference's own fp32 logits then depend on its fp32
        # rounding.  The reference's error is measured against its own float64 run; the GPU test compares two fp32
        # computations (the recorded one and the engine's), each with an error of that size, within logits_tol(lr).  A
        # waveform on which the reference's fp32 run is off by more than half that bound cannot test at that bound
        # (seed 151 at N = 10960 is one: 1.1e-4 .. 1.5e-4 from step 1 on, one conv weight element): take the next seed.
        while (logits[0].shape[0] == 1 and any(int(logits[i].argmax(-1)[0]) == 0 for i in range(steps + 1))) or \
                ref_err.max() > 0.5 * logits_tol(lr):
            print("  skip seed", seed, "ref fp32-vs-fp64", ref_err)
            seed += 100
            x, logits, final, names, ref_err = attempt()
        eff = adapter_effect(cfg, sd, x, logits[0])
        assert eff > 100 * logits_tol(lr), (tag, n, eff)
        out = {"weights_sha256": np.array(mg.weights_digest(sd)), "hp_json": np.array(repr(hp)),
               "steps": np.array(steps), "x": x, "logits": np.stack([logits[i] for i in range(steps + 1)]),
               "entries": np.array(names), "adapter_effect": np.array(eff), "wave_seed": np.array(seed),
               "ref_f32_err": ref_err}
        for k, v in final.items():
            out[f"final/{k}"] = v
        fn = f"g15_adapter_{tag}_N{n}{'_biasonly' if bias_only else ''}.npz"
        np.savez_compressed(os.path.join(HERE, fn), **out)
        print(fn, "T =", logits[0].shape[0], "seed", seed, "adapter_effect", eff, "ref fp32-vs-fp64", ref_err.max(),
              os.path.getsize(os.path.join(HERE, fn)))


def wide_cfg(hidden):
    """tests/test_gpu_headdim.py::wide_cfg with the MMS adapter."""
    cfg = get_config("wav2vec2-xls-r-1b")
    cfg.update(hidden_size=hidden, num_attention_heads=16, num_conv_pos_embedding_groups=16, num_hidden_layers=1,
               intermediate_size=256, conv_dim=[32] * 7, adapter_attn_dim=16)
    return cfg


def wide(ref):
    for hidden in (1024, 1280, 2048):
        cfg = wide_cfg(hidden)
        sd = synth_weights(cfg)
        seed = 160
        x = mg.wave(32000, seed)
        logits, _, names = mg.run_ref_suta(ref, cfg, sd, x, 2, lr=2e-5)
        eff = adapter_effect(cfg, sd, x, logits[0])
        assert eff > 100 * 5e-5, (hidden, eff)
        fn = f"g15_adapter_h{hidden}_a16_N32000.npz"
        np.savez_compressed(os.path.join(HERE, fn), weights_sha256=np.array(mg.weights_digest(sd)),
                            wave=np.array([32000, seed]), logits=np.stack([logits[i] for i in range(3)]),
                            adapter_effect=np.array(eff))
        print(fn, "adapter_effect", eff, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref = mg.import_reference()
    for w in sys.argv[1:] or ["keys", "tiny", "wide"]:
        if w.startswith("tiny:"):   # one tiny fixture by tag, e.g. tiny:tiny_h72_a16
            tiny(ref, only=w[5:])
        else:
            globals()[w](ref)
