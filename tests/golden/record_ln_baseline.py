"""g18_ln_parent.npz: logits and adapted tensors of a matrix of two-step adaptations that reaches every LayerNorm
kernel family and launch form, for the bitwise check of tests/test_gpu_ln_routes.py.

Needs an MI355X and the built library of the commit to record (the committed file was recorded with the commit before
the LayerNorm launches were described by LnSite / ln_route: the routes must reproduce every choice of the launchers
they replaced):
    python tests/golden/record_ln_baseline.py [OUT.npz]

RUNS is the matrix; tests/test_gpu_ln_routes.py replays it through run().  Every model is cut to one encoder layer;
each run is two adaptation steps on a fresh engine and keeps the logits of steps 0 and 2, the sha256 of every
trainable tensor of every slot after the call and the sha256 of the seeded weights.  The recorder runs each entry
twice and requires a bitwise repeat.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import suta_loader  # noqa: E402

suta_loader.load()
from suta_amd import synth  # noqa: E402
from suta_amd.config import family, get_config  # noqa: E402
from suta_amd.engine import SutaEngine, SutaHParams  # noqa: E402
from suta_amd.weights import synth_weights  # noqa: E402

FIXTURE = os.path.join(HERE, "g18_ln_parent.npz")

# every switch a run may set: cleared before each run, so a run sees its own settings and the defaults
SWITCHES = ("SUTA_CONV_Z_BF16", "SUTA_DY_PLANES", "SUTA_CONV_DX_PLANES", "SUTA_CONV_PLANES", "SUTA_FUSED_CONV_LN",
            "SUTA_BF16_PLANES", "SUTA_FAST_GELU", "SUTA_LN_RPW")

LONG = (32000, 20000)  # conv0 has 6399 rows: at or above the 4096-row switch of the conv partials' chunk size; T = 99 / 62
SHORT = (8000, 5000)   # 1599 rows: below it
ONE = (8000,)
FP32, BF16 = "fp32", "bf16"


def _run(name, model, precision, samples, env=None, **hp):
    return dict(name=name, model=model, precision=precision, samples=tuple(samples), env=dict(env or {}), hp=hp)


RUNS = [
    # scalar kernels: D <= 256 (NPL 4), the unfused layer-mode conv LayerNorm + launch_colsum, D = 1280 (NPL 32; in
    # bf16 mode with the bf16 copy written by a separate launch_to_bf16 pass)
    _run("tiny-group-fp32", "tiny-group", FP32, ONE),
    _run("tiny-layer-fp32-short", "tiny-layer", FP32, SHORT),
    _run("xlsr1b-bf16", "wav2vec2-xls-r-1b", BF16, ONE),
    # vectorised widths: conv width 512 in group mode (the post_aux operand) and H = 768 post-LN with stored x-hat;
    # H = 1024 stable with stored means
    _run("base-fp32-long", "wav2vec2-base", FP32, LONG),
    _run("base-bf16-long", "wav2vec2-base", BF16, LONG),
    # the fused conv backward, ktaps 0 and 10, in fp32 on both sides of the chunk-size switch, without and with the
    # conv bias gradient
    _run("d2v-base-fp32-long", "data2vec-audio-base", FP32, LONG),
    _run("d2v-base-fp32-short", "data2vec-audio-base", FP32, SHORT),
    _run("large-fp32-long", "wav2vec2-large", FP32, LONG),
    _run("large-fp32-short", "wav2vec2-large", FP32, SHORT),
    # the plane forms: wav2vec2-large in bf16 at its defaults and with each switch alone
    _run("large-bf16-long", "wav2vec2-large", BF16, LONG),
    _run("large-bf16-short", "wav2vec2-large", BF16, SHORT),
    _run("large-bf16-convzbf16-0", "wav2vec2-large", BF16, SHORT, {"SUTA_CONV_Z_BF16": "0"}),
    _run("large-bf16-dyplanes-0", "wav2vec2-large", BF16, SHORT, {"SUTA_DY_PLANES": "0"}),
    _run("large-bf16-convdxplanes-0", "wav2vec2-large", BF16, SHORT, {"SUTA_CONV_DX_PLANES": "0"}),
    _run("large-bf16-convplanes-0", "wav2vec2-large", BF16, SHORT, {"SUTA_CONV_PLANES": "0"}),
    _run("large-bf16-fusedconvln-0", "wav2vec2-large", BF16, SHORT, {"SUTA_FUSED_CONV_LN": "0"}),
    _run("large-bf16-planes-0", "wav2vec2-large", BF16, SHORT, {"SUTA_BF16_PLANES": "0"}),
    _run("large-bf16-fastgelu-0", "wav2vec2-large", BF16, SHORT, {"SUTA_FAST_GELU": "0"}),
    _run("large-bf16-lnrpw-1", "wav2vec2-large", BF16, SHORT, {"SUTA_LN_RPW": "1"}),
    # the rest: the positional stack's LayerNorm -> GELU, a frozen feature encoder, biases only
    _run("tiny-d2v-fp32", "tiny-d2v", FP32, ONE),
    _run("large-fp32-short-frozen-features", "wav2vec2-large", FP32, SHORT, train_feature=False),
    _run("base-fp32-biasonly", "wav2vec2-base", FP32, ONE, bias_only=True),
]


def check_coverage(runs):
    """A condition on the matrix (configs and switches, no GPU): every class of LayerNorm launch is present."""
    names = [r["name"] for r in runs]
    assert len(set(names)) == len(names), "duplicate run names"
    for r in runs:
        assert set(r["env"]) <= set(SWITCHES), r["name"]
        assert max(r["samples"]) <= 32000, r["name"]  # T <= 99

    def has(what, pred):
        assert any(pred(r, get_config(r["model"])) for r in runs), "no run with " + what

    layer = lambda c: c["feat_extract_norm"] == "layer"  # noqa: E731
    plain = lambda r: not r["env"] and not r["hp"]  # noqa: E731
    rows0 = lambda r: (max(r["samples"]) - 10) // 5 + 1  # noqa: E731  conv0 frames of the layout
    has("D <= 256", lambda r, c: c["hidden_size"] <= 256 and max(c["conv_dim"]) <= 256)
    has("the unfused layer-mode conv LayerNorm", lambda r, c: layer(c) and c["conv_dim"][0] != 512 and c["conv_bias"])
    has("NPL 32 in bf16 mode", lambda r, c: 1024 < c["hidden_size"] <= 2048 and r["precision"] == BF16)
    has("group-mode conv width 512 (post_aux)", lambda r, c: not layer(c) and c["conv_dim"][-1] == 512)
    for prec in (FP32, BF16):
        has("H = 768 post-LN in " + prec, lambda r, c: c["hidden_size"] == 768 and not c["do_stable_layer_norm"] and
            r["precision"] == prec and family(c) == "wav2vec2")
    has("H = 768 post-LN data2vec-audio", lambda r, c: c["hidden_size"] == 768 and family(c) == "data2vec-audio")
    has("H = 1024 stable", lambda r, c: c["hidden_size"] == 1024 and c["do_stable_layer_norm"])
    for big in (True, False):
        for bias in (True, False):  # the fused conv backward in fp32, ktaps 0 and 10 (conv0's kernel is 10 wide)
            has("the fp32 fused conv backward, rows %s 4096, conv bias %s" % (">=" if big else "<", bias),
                lambda r, c: layer(c) and c["conv_dim"] == [512] * 7 and c["conv_kernel"][0] == 10 and plain(r) and
                r["precision"] == FP32 and (rows0(r) >= 4096) == big and c["conv_bias"] == bias)
        has("wav2vec2-large in bf16 at its defaults, rows %s 4096" % (">=" if big else "<"),
            lambda r, c: r["model"] == "wav2vec2-large" and r["precision"] == BF16 and plain(r) and
            (rows0(r) >= 4096) == big)
    for sw, v in (("SUTA_CONV_Z_BF16", "0"), ("SUTA_DY_PLANES", "0"), ("SUTA_CONV_DX_PLANES", "0"),
                  ("SUTA_CONV_PLANES", "0"), ("SUTA_FUSED_CONV_LN", "0"), ("SUTA_BF16_PLANES", "0"),
                  ("SUTA_FAST_GELU", "0"), ("SUTA_LN_RPW", "1")):
        has(sw + "=" + v + " alone", lambda r, c: r["model"] == "wav2vec2-large" and r["precision"] == BF16 and
            r["env"] == {sw: v} and not r["hp"])
    has("wav2vec2-base in bf16", lambda r, c: r["model"] == "wav2vec2-base" and r["precision"] == BF16)
    has("the positional stack (ln_gelu)", lambda r, c: family(c) == "data2vec-audio" and c["hidden_size"] <= 256)
    has("train_feature=False", lambda r, c: r["hp"] == {"train_feature": False})
    has("bias_only=True", lambda r, c: r["hp"] == {"bias_only": True})


def weights_digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def run(run, setenv=None, delenv=None):
    """Two SUTA steps of `run` on a fresh engine: {"logits": steps 0 and 2 of every utterance, concatenated over frames,
    "params_sha256": of every trainable tensor of every slot, "weights_sha256"}.  setenv / delenv: the caller's way to
    change the environment (pytest's monkeypatch), os.environ by default."""
    setenv = setenv or os.environ.__setitem__
    delenv = delenv or (lambda k: os.environ.pop(k, None))
    for k in SWITCHES:
        delenv(k)
    for k, v in run["env"].items():
        setenv(k, v)
    cfg = dict(get_config(run["model"]))
    cfg["num_hidden_layers"] = 1
    sd = synth_weights(cfg)
    samples = run["samples"]
    eng = SutaEngine(cfg, sd, max_batch=len(samples), max_samples=max(samples))
    try:
        eng.set_precision(run["precision"])
        waves = [synth.wave(n, 180 + i) for i, n in enumerate(samples)]
        logits, _, _ = eng.adapt_varlen(waves, 2, SutaHParams(**run["hp"]), record=[0, 2])
        h = hashlib.sha256()
        for slot in range(len(samples)):
            for name in eng.trainable_names():
                h.update(f"{slot}/{name}".encode())
                h.update(eng.get_param(slot, name).tobytes())
    finally:
        eng.close()
        for k in run["env"]:
            delenv(k)
    return {"logits": np.concatenate([logits[r][u] for r in (0, 2) for u in range(len(samples))]),
            "params_sha256": h.hexdigest(), "weights_sha256": weights_digest(sd)}


def main(path):
    import time
    check_coverage(RUNS)
    out = {}
    for r in RUNS:
        t0 = time.time()
        a, b = run(r), run(r)
        assert np.array_equal(a["logits"], b["logits"]) and a["params_sha256"] == b["params_sha256"], r["name"]
        for k, v in a.items():
            out[r["name"] + "/" + k] = np.asarray(v)
        print(r["name"], a["logits"].shape, "%.1f s" % (time.time() - t0), flush=True)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
