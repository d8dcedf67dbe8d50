"""g16_w2v2_posconv_parent.npz: the wav2vec2 positional conv's logits as the engine computes them, for the bitwise check
of tests/test_gpu_families.py::test_wav2vec2_positional_conv_is_bitwise_the_parent_commits.

Needs an MI355X and the built library of the commit to record (the committed file was recorded with the commit before
data2vec-audio's stack epilogues were compiled into posconv_kernel):
    python tests/golden/record_posconv_baseline.py [OUT.npz]

tiny-layer runs the positional conv on the conv-A GEMM (group width 16), the one-layer H = 768 model of
tests/test_gpu_headdim.py::wide_cfg on posconv_kernel (group width 48, K = 128): 2 steps at the default hparams, logits
of steps 0..2, each model run twice on fresh engines and required to repeat bitwise.
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
from suta_amd.config import get_config  # noqa: E402
from suta_amd.engine import SutaEngine, SutaHParams  # noqa: E402
from suta_amd.weights import synth_weights  # noqa: E402


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def main(path):
    out = {}
    wide = get_config("wav2vec2-xls-r-1b")
    wide.update(hidden_size=768, num_attention_heads=16, num_conv_pos_embedding_groups=16, num_hidden_layers=1,
                intermediate_size=256, conv_dim=[32] * 7)
    for key, cfg, n, seed in (("tiny-layer", get_config("tiny-layer"), 32000, 191), ("w2v2h768", wide, 48000, 192)):
        sd = synth_weights(cfg)
        runs = []
        for _ in range(2):
            eng = SutaEngine(cfg, sd, max_batch=1, max_samples=64000)
            logits, _, T = eng.adapt(synth.wave(n, seed), 2, SutaHParams(), record=[0, 1, 2])
            eng.close()
            runs.append(np.stack([logits[r][0] for r in (0, 1, 2)]))
        assert np.array_equal(runs[0], runs[1]), key
        out[f"{key}/weights_sha256"] = np.array(digest(sd))
        out[f"{key}/wave"] = np.array([n, seed])
        out[f"{key}/logits"] = runs[0]
        print(key, "T =", T, runs[0].shape)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g16_w2v2_posconv_parent.npz"))
