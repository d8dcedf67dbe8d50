"""GPU tier: a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run as its own process, the real
engine on a tiny model: one JSON line with the headline keys and none of --full's objects, and the dumped arrays
equal what the engine returns for the last timed step's utterances (graph replay in the bench, the first eager
call here: bitwise equal ids and logits, as tests/test_gpu_bench_scale.py pins at the bench's own size).  CPU form
with a stand-in engine: tests/test_bench_plain.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.multirank import REPO

pytestmark = pytest.mark.gpu


def test_plain_bench_dumps_the_last_timed_step(tmp_path):
    import bench
    from suta_amd import synth
    from suta_amd.config import get_config
    from suta_amd.engine import SutaEngine, SutaHParams
    from suta_amd.weights import synth_weights
    B, N, S, steps, warmup = 3, 8000, 10, 2, 1
    out_dir = tmp_path / "out"
    argv = [sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--model", "tiny-group",
            "--batch", str(B), "--n-samples", str(N), "--suta-steps", str(S), "--steps", str(steps),
            "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    p = subprocess.run(argv, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, f"{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(B * steps / (out["ms_per_step"] * steps / 1000), rel=1e-2)
    assert out["unit"] == "utt/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    for k in ("roofline", "time_breakdown_ms", "batch64", "fp32_split_bf16", "cpu_baseline", "c4", "c5"):
        assert k not in out
    cfg = get_config("tiny-group")
    eng = SutaEngine(cfg, synth_weights(cfg), device=0, max_batch=B, max_samples=N)
    x = synth.batch(N, B, start=(warmup + steps - 1) * B)
    logits, ids, T = eng.adapt(x, S, SutaHParams(), record=bench.RECORD)
    eng.close()
    assert sorted(os.listdir(out_dir)) == sorted(
        ["frames.npy", "logits_utterances.npy"] + [f"ids_step{r:02d}.npy" for r in bench.RECORD]
        + [f"logits_step{r:02d}.npy" for r in bench.RECORD])
    np.testing.assert_array_equal(np.load(out_dir / "frames.npy"), np.array([T], np.float32))
    np.testing.assert_array_equal(np.load(out_dir / "logits_utterances.npy"), np.arange(B, dtype=np.float32))
    for r in bench.RECORD:
        got = np.load(out_dir / f"ids_step{r:02d}.npy")
        assert got.dtype == np.float32 and got.shape == (B, T)
        np.testing.assert_array_equal(got, ids[r])
        lg = np.load(out_dir / f"logits_step{r:02d}.npy")
        assert lg.dtype == np.float32 and lg.shape == (B, T, cfg["vocab_size"])
        np.testing.assert_array_equal(lg, logits[r])
        np.testing.assert_array_equal(got, lg.argmax(-1))
