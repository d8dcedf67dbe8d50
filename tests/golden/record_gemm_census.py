"""g17_gemm_census_parent.json: which GEMM kernel, tile, grid, split count and epilogue every launch of a small matrix
of one-step adaptations takes (the engine's GEMM census, without its "ms|" timing entries), for the exact comparison
of tests/test_gpu_gemm_routes.py.

Needs an MI355X and the built library of the commit to record (the committed file was recorded with the commit before
the GEMM dispatcher computed a route: the route must reproduce every choice of the code it replaced):
    python tests/golden/record_gemm_census.py [OUT.json]

RUNS is the matrix; tests/test_gpu_gemm_routes.py replays it through run_census().  The census shows neither the
main-loop form nor the tile order; the bitwise tests of tests/test_gpu_large_bf16.py and tests/test_gpu_f32_256.py
cover those.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import suta_loader  # noqa: E402

suta_loader.load()
from suta_amd import synth  # noqa: E402
from suta_amd.config import get_config  # noqa: E402
from suta_amd.engine import SutaEngine, SutaHParams  # noqa: E402
from suta_amd.weights import synth_weights  # noqa: E402

FIXTURE = os.path.join(HERE, "g17_gemm_census_parent.json")

# every switch a run may set: cleared before each run, so a run sees its own settings and the defaults
SWITCHES = ("SUTA_F32P", "SUTA_HBX", "SUTA_HBX_T", "SUTA_HBX_FORM", "SUTA_HBT4", "SUTA_HBP_CONV", "SUTA_EPI_FAST",
            "SUTA_SPLITK", "SUTA_BF16_PLANES", "SUTA_POSCONV")

PAIR = (32000, 20000)  # ragged pair: T = 99 / 62, edge tiles in every GEMM
FP32, X6, BF16 = "fp32", "fp32-split-bf16", "bf16"


def _run(name, model, precision, samples, env=None, layers=None):
    return dict(name=name, model=model, precision=precision, samples=tuple(samples), env=dict(env or {}),
                layers=layers)


# (model cut to `layers` encoder layers; one sample count: adapt on that many equal utterances' worth given as
# (n,) * B; unequal counts: adapt_varlen)
RUNS = [
    # defaults in all three precisions: the tiny presets, the one-layer base / large models on the ragged pair
    _run("tiny-group-fp32", "tiny-group", FP32, (8000,)),
    _run("tiny-group-x6", "tiny-group", X6, (8000,)),
    _run("tiny-group-bf16", "tiny-group", BF16, (8000,)),
    _run("tiny-layer-fp32-pair", "tiny-layer", FP32, (8000, 5000)),
    _run("tiny-hubert-bf16-pair", "tiny-hubert", BF16, (8000, 5000)),
    _run("base1-fp32-pair", "wav2vec2-base", FP32, PAIR, layers=1),
    _run("base1-x6-pair", "wav2vec2-base", X6, PAIR, layers=1),
    _run("large1-bf16-pair", "wav2vec2-large", BF16, PAIR, layers=1),
    _run("large1-fp32-pair", "wav2vec2-large", FP32, PAIR, layers=1),
    # batch 64 x 32000 samples: grids that reach the ">= 256 tiles of 256^2" thresholds without forcing
    _run("base1-fp32-b64", "wav2vec2-base", FP32, (32000,) * 64, layers=1),
    _run("base1-x6-b64", "wav2vec2-base", X6, (32000,) * 64, layers=1),
    _run("large1-bf16-b64", "wav2vec2-large", BF16, (32000,) * 64, layers=1),
    # the switches
    _run("large1-fp32-pair-f32p2", "wav2vec2-large", FP32, PAIR, {"SUTA_F32P": "2"}, 1),
    _run("base1-fp32-pair-f32p2", "wav2vec2-base", FP32, PAIR, {"SUTA_F32P": "2"}, 1),
    _run("base1-fp32-b64-f32p0", "wav2vec2-base", FP32, (32000,) * 64, {"SUTA_F32P": "0"}, 1),
    _run("large1-bf16-pair-hbx2", "wav2vec2-large", BF16, PAIR, {"SUTA_HBX": "2"}, 1),
    _run("large1-bf16-b64-hbx0", "wav2vec2-large", BF16, (32000,) * 64, {"SUTA_HBX": "0"}, 1),
    _run("large1-bf16-pair-hbx2-t0", "wav2vec2-large", BF16, PAIR, {"SUTA_HBX": "2", "SUTA_HBX_T": "0"}, 1),
    _run("large1-bf16-pair-hbx2-t1", "wav2vec2-large", BF16, PAIR, {"SUTA_HBX": "2", "SUTA_HBX_T": "1"}, 1),
    _run("large1-bf16-pair-hbx2-form0", "wav2vec2-large", BF16, PAIR, {"SUTA_HBX": "2", "SUTA_HBX_FORM": "0"}, 1),
    _run("large1-bf16-pair-hbt4-2", "wav2vec2-large", BF16, PAIR, {"SUTA_HBT4": "2"}, 1),
    _run("large1-bf16-b64-hbt4-0", "wav2vec2-large", BF16, (32000,) * 64, {"SUTA_HBT4": "0"}, 1),
    _run("large1-bf16-pair-hbx2-hbpconv0", "wav2vec2-large", BF16, PAIR, {"SUTA_HBX": "2", "SUTA_HBP_CONV": "0"}, 1),
    _run("large1-bf16-b64-hbpconv0", "wav2vec2-large", BF16, (32000,) * 64, {"SUTA_HBP_CONV": "0"}, 1),
    _run("large1-bf16-pair-hbx2-epifast0", "wav2vec2-large", BF16, PAIR, {"SUTA_HBX": "2", "SUTA_EPI_FAST": "0"}, 1),
    # (full grids without the 32-bit-offset epilogue, or without the staged C^T epilogue: the GELU linears' rule)
    _run("large1-bf16-b64-epifast0", "wav2vec2-large", BF16, (32000,) * 64, {"SUTA_EPI_FAST": "0"}, 1),
    _run("large1-bf16-b64-hbxt1", "wav2vec2-large", BF16, (32000,) * 64, {"SUTA_HBX_T": "1"}, 1),
    _run("large1-bf16-b64-hbxt0", "wav2vec2-large", BF16, (32000,) * 64, {"SUTA_HBX_T": "0"}, 1),
    _run("base1-fp32-pair-f32p2-epifast0", "wav2vec2-base", FP32, PAIR, {"SUTA_F32P": "2", "SUTA_EPI_FAST": "0"}, 1),
    _run("base1-fp32-pair-splitk0", "wav2vec2-base", FP32, PAIR, {"SUTA_SPLITK": "0"}, 1),
    _run("large1-bf16-pair-splitk0", "wav2vec2-large", BF16, PAIR, {"SUTA_SPLITK": "0"}, 1),
    _run("large1-bf16-pair-planes0", "wav2vec2-large", BF16, PAIR, {"SUTA_BF16_PLANES": "0"}, 1),
    _run("large1-bf16-b64-planes0", "wav2vec2-large", BF16, (32000,) * 64, {"SUTA_BF16_PLANES": "0"}, 1),
    _run("tiny-d2v-fp32-posconv0", "tiny-d2v", FP32, (8000,), {"SUTA_POSCONV": "0"}),
    _run("tiny-d2v-bf16-posconv0", "tiny-d2v", BF16, (8000, 5000), {"SUTA_POSCONV": "0"}),
]


def run_census(run, setenv=None, delenv=None):
    """One SUTA step of `run` with the census on; the census without its timing entries.  setenv / delenv: the
    caller's way to change the environment (pytest's monkeypatch), os.environ by default."""
    setenv = setenv or os.environ.__setitem__
    delenv = delenv or (lambda k: os.environ.pop(k, None))
    for k in SWITCHES:
        delenv(k)
    for k, v in run["env"].items():
        setenv(k, v)
    cfg = dict(get_config(run["model"]))
    if run["layers"]:
        cfg["num_hidden_layers"] = run["layers"]
    samples = run["samples"]
    eng = SutaEngine(cfg, synth_weights(cfg), max_batch=len(samples), max_samples=max(samples))
    try:
        eng.set_precision(run["precision"])
        eng.set_census(True)
        waves = [synth.wave(n, 170 + i) for i, n in enumerate(samples)]
        if len(set(samples)) == 1:
            eng.adapt(np.stack(waves), 1, SutaHParams(), record=[1], want_logits=False)
        else:
            eng.adapt_varlen(waves, 1, SutaHParams(), record=[1], want_logits=False)
        census = eng.get_census()
        eng.set_census(False)
    finally:
        eng.close()
        for k in run["env"]:
            delenv(k)
    return {k: v for k, v in census.items() if not k.startswith("ms|")}


def check_coverage(all_runs):
    """The union of the runs reaches every kernel family the engine can reach (gbf_x6 and hbx16 exist only behind
    gemm_set_variant), split-K, both conv-A forms and batched GEMMs."""
    keys = set()
    for c in all_runs.values():
        keys.update(k for k in c if not k.startswith(("grid ", "epi ")))
    fams = {k.split(" ", 1)[0] for k in keys}
    for want in ("f32p", "x6", "x6_1plane", "gbf", "hb", "hbt", "hbt4", "hbx"):
        assert want in fams, (want, sorted(fams))
    assert fams & {"f32", "glds"}, sorted(fams)
    assert fams <= {"f32", "glds", "f32p", "x6", "x6_1plane", "gbf", "hb", "hbt", "hbt4", "hbx"}, sorted(fams)

    def field(k, name):
        return int(next(w for w in k.split() if w.startswith(name + "=")).split("=")[1])

    assert any(field(k, "split") > 1 for k in keys), "no split-K launch"
    assert any(field(k, "z") > 1 for k in keys), "no batched launch"
    assert any(k.endswith(" conv") for k in keys), "no conv-A launch"
    assert any(k.endswith(" conv-seg") for k in keys), "no conv-A launch with weight segments"
    assert any(k.startswith("hbx ") and field(k, "z") > 1 for k in keys), "no batched hbx launch"
    assert any(k.startswith("hbx ") and k.endswith(" conv-seg") for k in keys), "no hbx CONV-form launch"


def main(path):
    import time
    out = {}
    for run in RUNS:
        t0 = time.time()
        out[run["name"]] = run_census(run)
        print(run["name"], len(out[run["name"]]), "entries", "%.1f s" % (time.time() - t0), flush=True)
    check_coverage(out)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
