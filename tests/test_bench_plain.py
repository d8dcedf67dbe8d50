"""CPU tier: what a plain `bench.py --gpus 1 --steps K --warmup W` run does and what `--full` and
`--dump-outputs DIR` add, through bench.run() with a stand-in engine (the real engine: tests/test_gpu_bench_plain.py).

* plain: W + K adapt calls and nothing else (no timing pass, no other precision, no CPU baseline), the headline keys;
* --full: the per-kernel pass and the split-bf16 line are back in the JSON line;
* --dump-outputs: the arrays the last timed call returned and the logits of its untimed repeat, float32, identical
  from run to run; logits over the size limit are cut to a seeded sample of the utterances;
* the bench's threaded input generation equals synth.batch."""
import contextlib
import io
import json

import numpy as np

import bench
from suta_amd import synth

B, N, K, W = 3, 4000, 3, 2
ARGV = ["--gpus", "1", "--model", "tiny-group", "--batch", str(B), "--n-samples", str(N), "--suta-steps", "2",
        "--steps", str(K), "--warmup", str(W)]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "time_breakdown_ms", "frontend", "attention", "batch64", "fp32_split_bf16", "cpu_baseline",
             "c4", "c5")


class Engine:
    """Stand-in: ids derived from the waveform it is given; counts its calls by kind."""
    T, V = 12, 5

    def __init__(self):
        self.calls, self.logit_calls, self.timing_passes, self.precisions = [], [], 0, []

    def set_precision(self, mode):
        self.precisions.append(mode)

    def adapt(self, wav, steps, hp, record=(), want_logits=True):
        w = np.asarray(wav)
        (self.logit_calls if want_logits else self.calls).append(float(w[0, 0]))
        logits = {r: np.sin(w[:, :self.T, None] * (r + 1) + np.arange(self.V, dtype=np.float32)) for r in record}
        ids = {r: a.argmax(-1).astype(np.int32) for r, a in logits.items()}
        return (logits if want_logits else None), ids, self.T

    def sync(self):
        pass

    def close(self):
        pass

    # per-kernel pass (--full only)
    def set_timing(self, on):
        self.timing_passes += bool(on)

    def get_timing(self):
        return {f: (1.0, 4) for f in ("gemm", "attention", "frontend")}

    def get_timing_ex(self):
        return {f: (1.0, 4, 4096.0) for f in ("gemm", "attention", "frontend")}


def run_bench(argv):
    eng = Engine()
    args = bench.build_parser().parse_args(argv)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ret = bench.run(args, 0, 1, bench.Comm(), bench.Device(None), lambda cfg, b, n: eng)
    lines = [ln for ln in buf.getvalue().splitlines() if ln.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == ret
    return ret, eng


def test_plain_run_is_the_headline_alone():
    out, eng = run_bench(ARGV)
    assert len(eng.calls) == W + K and not eng.logit_calls    # warm-up + timed steps, nothing after them
    assert eng.timing_passes == 0 and eng.precisions == ["fp32"]
    assert all(k in out for k in HEADLINE) and not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == K and out["warmup"] == W and out["unit"] == "utt/s" and out["higher_is_better"] is True
    assert out["value"] > 0 and out["ms_per_step"] >= 0
    # each step its own utterances, in order
    assert eng.calls == [float(synth.wave(N, i * B)[0]) for i in range(W + K)]


def test_full_brings_back_the_other_measurements():
    out, eng = run_bench(ARGV + ["--full", "--no-cpu-baseline"])
    assert all(k in out for k in HEADLINE)
    assert out["roofline"]["launches"] == 4 and "time_breakdown_ms" in out and out["attention"]["tflops"] > 0
    assert out["fp32_split_bf16"]["precision"] == "fp32-split-bf16" and "roofline" in out["fp32_split_bf16"]
    assert eng.timing_passes == 2 and eng.precisions == ["fp32", "fp32-split-bf16", "fp32"]
    # the --no-... switches still take their parts out
    out, eng = run_bench(ARGV + ["--full", "--no-cpu-baseline", "--no-timing", "--no-split"])
    assert not [k for k in FULL_ONLY if k in out] and len(eng.calls) == W + K


def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _, eng = run_bench(ARGV + ["--dump-outputs", a])
    run_bench(ARGV + ["--dump-outputs", b])
    last = synth.batch(N, B, start=(W + K - 1) * B)      # the last timed step's utterances
    assert len(eng.calls) == W + K and eng.logit_calls == [float(last[0, 0])]   # one untimed repeat, for the logits
    logits, want, T = Engine().adapt(last, 2, None, record=bench.RECORD)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(["frames.npy", "logits_utterances.npy"] + [f"ids_step{r:02d}.npy" for r in bench.RECORD]
                           + [f"logits_step{r:02d}.npy" for r in bench.RECORD])
    for r in bench.RECORD:
        got = np.load(tmp_path / "a" / f"ids_step{r:02d}.npy")
        assert got.dtype == np.float32 and got.shape == (B, T)
        np.testing.assert_array_equal(got, want[r])
        lg = np.load(tmp_path / "a" / f"logits_step{r:02d}.npy")
        assert lg.dtype == np.float32 and lg.shape == (B, T, Engine.V)
        np.testing.assert_array_equal(lg, logits[r].astype(np.float32))
        for n in (f"ids_step{r:02d}.npy", f"logits_step{r:02d}.npy"):
            np.testing.assert_array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "frames.npy"), np.array([T], np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "logits_utterances.npy"), np.arange(B, dtype=np.float32))
    # another number of timed steps ends on other utterances
    c = str(tmp_path / "c")
    run_bench(ARGV[:-4] + ["--steps", str(K + 1), "--warmup", str(W), "--dump-outputs", c])
    assert not np.array_equal(np.load(tmp_path / "c" / "ids_step00.npy"), np.load(tmp_path / "a" / "ids_step00.npy"))


def test_threaded_input_generation_equals_synth_batch():
    starts = [0, 5, 40]
    got = list(bench.synth_batches(1000, 5, starts))
    assert len(got) == 3
    for g, s in zip(got, starts):
        assert g.dtype == np.float32
        np.testing.assert_array_equal(g, synth.batch(1000, 5, start=s))


def test_dump_outputs_samples_logits_over_the_limit(tmp_path, monkeypatch):
    per_utt = len(bench.RECORD) * Engine.T * Engine.V * 4
    monkeypatch.setattr(bench, "DUMP_LOGITS_BYTES", 2 * per_utt + 1)      # room for 2 of the 3 utterances
    for d in ("a", "b"):
        run_bench(ARGV + ["--dump-outputs", str(tmp_path / d)])
    rows = np.load(tmp_path / "a" / "logits_utterances.npy")
    assert len(rows) == 2 and len(set(rows)) == 2 and set(rows) <= {0.0, 1.0, 2.0}
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "logits_utterances.npy"))
    last = synth.batch(N, B, start=(W + K - 1) * B)
    logits, _, _ = Engine().adapt(last, 2, None, record=bench.RECORD)
    for r in bench.RECORD:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"logits_step{r:02d}.npy"),
                                      logits[r][rows.astype(int)].astype(np.float32))
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) < 64 << 20
