"""GPU tier: the exact-fp32 GEMMs on the four-phase 256 x 256 kernel (gemm_hbp_kernel's fp32 forms, census name
"f32p") against the 128 x 128 LDS-DMA kernel (gemm_glds_kernel) they replace.

Both issue the same v_mfma_f32_32x32x2_f32 products in the same k order and apply the same epilogue operations in
the same order, so with split-K off (a split sums k in another order) every logit and every adapted tensor is
bitwise equal.  SUTA_F32P=2 forces the new kernel on every eligible GEMM of a ragged pair (T = 99 / 62: 198 rows of a
256-row tile, conv lengths 3199 ... 99 -- edge tiles by construction); the default switch is checked on a batch whose
first conv GEMM fills one round of 256 tiles.
"""
import numpy as np
import pytest

from suta_amd import synth
from suta_amd.config import get_config
from suta_amd.engine import SutaEngine, SutaHParams
from suta_amd.weights import synth_weights

pytestmark = pytest.mark.gpu


def _run(monkeypatch, cfg, sd, waves, steps, f32p, max_batch):
    if f32p is None:
        monkeypatch.delenv("SUTA_F32P", raising=False)
    else:
        monkeypatch.setenv("SUTA_F32P", f32p)
    eng = SutaEngine(cfg, sd, max_batch=max_batch, max_samples=32000)
    eng.set_precision("fp32")
    eng.set_census(True)
    logits, _, T = eng.adapt_varlen(waves, steps, SutaHParams(), record=[0, steps])
    census = eng.get_census()
    eng.set_census(False)
    params = [{n: eng.get_param(u, n) for n in eng.trainable_names()} for u in range(len(waves))]
    eng.close()
    return logits, params, census, T


@pytest.mark.parametrize("model", ["wav2vec2-base", "wav2vec2-large"])
def test_f32_256_tile_kernel_bitwise_equals_128_tile(monkeypatch, model):
    """wav2vec2-base (GroupNorm conv stack: bias-free conv GEMMs with the GELU + pre-activation epilogue, GELU' input
    gradients; post-LN encoder) and wav2vec2-large (layer-norm conv stack with bias, stable-LN encoder), 3 SUTA steps
    in exact fp32 on a ragged pair: SUTA_F32P=2 against SUTA_F32P=0."""
    monkeypatch.setenv("SUTA_SPLITK", "0")
    cfg = get_config(model)
    sd = synth_weights(cfg)
    waves = [synth.wave(32000, 182), synth.wave(20000, 183)]
    ref_l, ref_p, ref_c, T = _run(monkeypatch, cfg, sd, waves, 3, "0", 2)
    new_l, new_p, census, T2 = _run(monkeypatch, cfg, sd, waves, 3, "2", 2)
    assert list(T) == [99, 62] and list(T2) == [99, 62]
    txt = "\n".join(f"{k}: {v}" for k, v in sorted(census.items()))
    assert not any(k.startswith("f32p ") for k in ref_c), ref_c
    f32p = [k for k in census if k.startswith("f32p 256x256 ")]
    assert any(" z=1 " in k and k.endswith(" NT") for k in f32p), txt                  # forward linears
    assert any(" z=1 " in k and k.endswith(" NN") for k in f32p), txt                  # the linears' input gradients
    assert any(" z=2 " in k and k.endswith(" NN") for k in f32p), txt                  # conv forward (per utterance)
    assert any(" z=2 " in k and k.endswith(" conv-seg") for k in f32p), txt            # conv input gradients
    for r in (0, 3):
        for u in range(2):
            assert np.array_equal(new_l[r][u], ref_l[r][u]), (r, u)
    for u in range(2):
        for n, v in new_p[u].items():
            assert np.array_equal(v, ref_p[u][n]), (u, n)


def test_f32_256_tile_kernel_default_switch_reaches_full_grids(monkeypatch):
    """Default switches: a GEMM moves to the 256 x 256 kernel once its grid holds one round of 256 tiles and the
    256-row tile pads it no more than the kernel gains.  Eleven utterances of 30 730 samples of wav2vec2-base: the
    second conv layer has 3072 rows per utterance (12 whole tiles), so its forward is 11 x 12 x 2 = 264 tiles and
    moves; the next layer's 1535 rows (6 tiles of 256 against 12 of 128, but 132 tiles in all) and the encoder's
    linears (11 x 95 rows) stay on the 128 x 128 kernel.  Bitwise against SUTA_F32P=0."""
    monkeypatch.setenv("SUTA_SPLITK", "0")
    cfg = get_config("wav2vec2-base")
    sd = synth_weights(cfg)
    waves = [synth.wave(30730, 190 + i) for i in range(11)]
    ref_l, ref_p, _, _ = _run(monkeypatch, cfg, sd, waves, 1, "0", 11)
    new_l, new_p, census, _ = _run(monkeypatch, cfg, sd, waves, 1, None, 11)
    txt = "\n".join(f"{k}: {v}" for k, v in sorted(census.items()))
    assert any(k.startswith("grid f32p 256x256 gx=2 gy=12 z=11 ") for k in census), txt
    assert not any(k.startswith("f32p ") and " z=1 " in k for k in census), txt
    assert not any(k.startswith("grid f32p 256x256 gx=2 gy=6 ") for k in census), txt
    for r in (0, 1):
        for u in range(11):
            assert np.array_equal(new_l[r][u], ref_l[r][u]), (r, u)
    for u in (0, 10):
        for n, v in new_p[u].items():
            assert np.array_equal(v, ref_p[u][n]), (u, n)
