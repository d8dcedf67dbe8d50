"""Loss-family time per SUTA step at two vocabulary sizes.

The base geometry with synthetic weights at vocab_size 32 (the one-block-per-utterance kernel) and 392 (the
any-vocabulary path, ops.hip loss_wide_*), B = 164 utterances of 8 s (T = 399), the bench.py workload.  Eager with
suta_set_timing: every launch is bracketed by HIP events and summed per kernel family.  Prints one JSON line per
vocabulary: the loss family's ms per step, and its share of all timed kernel time of the call (S steps = S backward
+ Adam + forward passes plus the initial forward).

usage: python tools/loss_bench.py [--batch 164] [--steps 3] [--vocab 32 392] [--wide]
       --wide sets SUTA_LOSS_WIDE=1 (the any-vocabulary path at vocab_size 32 too)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import suta_loader  # noqa: E402

suta_loader.load()
import torch  # noqa: E402
from suta_amd import synth  # noqa: E402
from suta_amd.config import get_config  # noqa: E402
from suta_amd.engine import SutaEngine, SutaHParams  # noqa: E402
from suta_amd.weights import synth_weights  # noqa: E402


def run(V, B, N, steps):
    cfg = get_config("wav2vec2-base")
    cfg["vocab_size"] = V
    eng = SutaEngine(cfg, synth_weights(cfg), device=0, max_batch=B, max_samples=N)
    x = torch.from_numpy(synth.batch(N, B, start=0)).to("cuda:0")
    hp = SutaHParams()
    eng.adapt(x, 1, hp, record=[1], want_logits=False)   # warm-up: workspace, code objects
    eng.set_timing(True)                                 # (zeroes the family counters)
    eng.adapt(x, steps, hp, record=[steps], want_logits=False)
    t = eng.get_timing_ex()
    eng.close()
    total = sum(v[0] for v in t.values())
    loss_ms, n_loss = t["loss"][0], t["loss"][1]
    return {"vocab_size": V, "batch": B, "steps": steps, "loss_ms_per_step": round(loss_ms / max(1, n_loss), 4),
            "kernel_ms_per_step": round(total / steps, 3), "loss_share": round(loss_ms / total, 6),
            "wide_forced": os.environ.get("SUTA_LOSS_WIDE", "0") not in ("", "0")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=164)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=128000)
    ap.add_argument("--vocab", type=int, nargs="+", default=[32, 392])
    ap.add_argument("--wide", action="store_true")
    a = ap.parse_args()
    if a.wide:
        os.environ["SUTA_LOSS_WIDE"] = "1"
    for V in a.vocab:
        r = run(V, a.batch, a.samples, a.steps)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
