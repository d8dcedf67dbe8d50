"""Attention time of one SUTA step on both paths, through the engine's timing families: the flash kernels (family
'attention' + the softmax-backward row term in 'softmax') against the P-storing path of SUTA_ATTN_FUSED=0 (the
attention GEMMs of the per-shape table + 'softmax': row softmax and row term).  One encoder layer at full width, tiny
conv stack and FFN, so the engine's other work stays small.  The timed call (one step, nothing recorded) runs 2
forwards and 1 backward of the layer: family 7 counts 3 launches, the backward with its dQ reduction being one.

Run: python tools/attn_paths.py [hidden=1280] [heads=16] [batch=164] [n_samples=128000] [precision=fp32]
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import suta_loader  # noqa: E402

suta_loader.load()
from suta_amd import synth  # noqa: E402
from suta_amd.config import get_config, num_frames  # noqa: E402
from suta_amd.engine import SutaEngine, SutaHParams  # noqa: E402
from suta_amd.weights import synth_weights  # noqa: E402


def main():
    a = sys.argv[1:]
    hidden, heads, B, n = (int(a[i]) if len(a) > i else v for i, v in enumerate((1280, 16, 164, 128000)))
    precision = a[4] if len(a) > 4 else "fp32"
    cfg = get_config("wav2vec2-xls-r-1b")
    cfg.update(hidden_size=hidden, num_attention_heads=heads, num_conv_pos_embedding_groups=16, num_hidden_layers=1,
               intermediate_size=256, conv_dim=[32] * 7)
    sd = synth_weights(cfg)
    T, d = num_frames(cfg, n), hidden // heads
    x = np.stack([synth.wave(n, 900 + (b % 8)) for b in range(B)])
    for fused in ("1", "0"):
        os.environ["SUTA_ATTN_FUSED"] = fused
        eng = SutaEngine(cfg, sd, max_batch=B, max_samples=n)
        eng.set_precision(precision)
        eng.set_graphs(False)
        eng.adapt(x, 1, SutaHParams(), record=[])     # warm-up (allocations, LDS attributes)
        eng.set_timing(True)
        eng.set_census(True)
        eng.adapt(x, 1, SutaHParams(), record=[])
        fam = eng.get_timing_ex()
        shapes = eng.get_gemm_shape_times()
        eng.set_census(False)
        eng.set_timing(False)
        gemm_ms, gemm_n = 0.0, 0
        for k, (cnt, ms) in shapes.items():
            m = tuple(int(re.search(rf"\b{c}=(\d+)", k).group(1)) for c in "MNK")
            if m in ((T, T, d), (T, d, T)):
                gemm_ms += ms
                gemm_n += cnt
        print(f"{precision} hidden={hidden} heads={heads} dh={d} B={B} T={T} SUTA_ATTN_FUSED={fused}: "
              f"attention family {fam['attention'][0]:.3f} ms ({fam['attention'][1]} launches), "
              f"attention GEMMs {gemm_ms:.3f} ms ({gemm_n} launches), softmax family {fam['softmax'][0]:.3f} ms "
              f"({fam['softmax'][1]} launches), total {fam['attention'][0] + gemm_ms + fam['softmax'][0]:.3f} ms, "
              f"workspace {eng.workspace_bytes() / 2 ** 20:.0f} MiB", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
