"""Golden vectors for CTC vocabularies other than the 32 letters, from the REFERENCE's own code.

Build container only (it reads the reference checkout through make_golden.py, whose helpers it imports):
    python tests/golden/make_golden_vocab.py

  g10_vocab_loss_v<V>.npz      loss + dL/dlogits through reference forward_and_adapt (main.py:172-215) on
                               the fake-logits module, one file per class count V:
                                 33 (the literal class_num=32 of mcc_loss no longer equals V), 64, 65
                                 (a second 64-class chunk with a one-element tail), 96, 392, 1024 (the cap),
                                 each at T = 1 and 7, plus one long shape (T = 130 at V = 96, 70 at 392,
                                 24 at 1024).  Per case: fp32 logits, the fp64 gradient and loss, hp, and the
                                 scalar ref_f32_relerr = max|grad_f32 - grad_f64| / max|grad_f64| of the
                                 reference's own fp32 run.
  g10_vocab_loss_v96_cases.npz V = 96, T = 49: all-blank (NaN loss), em_coef 1 and 0, no blank mask,
                               div_coef 0.4, and exact ties of the row maximum (columns 0 and 70 on some
                               rows, 5 and 80 on others: torch.argmax takes the first).
  g11_vocab_tiny_<variant>_N<n>.npz  tiny-config episodic SUTA (main.py:327-348) with a widened lm_head:
                               tiny-group at vocab_size 41 and tiny-layer at 392; 4 steps, lr 5e-4, the
                               scripts' flags: logits after every step + final trainable tensors.
  g12_vocab96.json             a synthetic 96-token vocab.json (multi-character tokens, <pad> at id 17)
  g12_ctc_decode_vocab96.json  HF Wav2Vec2CTCTokenizer.batch_decode of ~100 random id sequences on it
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


def ref_loss_grad(ref, L, em, rw, nb, div, temp=2.5):
    """(grad_f64, loss_f64, grad_f32) of the reference objective at logits L (1, T, V)."""
    res = {}
    for dt in (torch.float32, torch.float64):
        fake = mg._FakeLogits(torch.from_numpy(L).to(dt))
        grads, losses = [], []
        fake.L.register_post_accumulate_grad_hook(lambda p: grads.append(p.grad.detach().clone()))
        orig = torch.Tensor.backward

        def bw(self, *a, **k):
            losses.append(self.detach().clone())
            return orig(self, *a, **k)
        torch.Tensor.backward = bw
        try:
            opt = torch.optim.SGD([fake.L], lr=1.0)
            ref.forward_and_adapt(None, fake, opt, em, rw, temp, nb, None, div)
        finally:
            torch.Tensor.backward = orig
        res[dt] = (grads[0][0].numpy(), losses[0].item())
    g64, l64 = res[torch.float64]
    g32, _ = res[torch.float32]
    return g64, l64, g32


def _store(out, cases, name, L, g64, l64, g32, hp):
    out[f"{name}/logits"] = L[0]
    out[f"{name}/grad_f64"] = g64
    out[f"{name}/loss_f64"] = np.array(l64)
    gm = np.abs(g64).max()
    out[f"{name}/ref_f32_relerr"] = np.array(float(np.abs(g32.astype(np.float64) - g64).max() / gm) if gm > 0 else 0.0)
    out[f"{name}/hp"] = np.array(hp)
    cases.append(name)


def g10(ref):
    long_T = {96: 130, 392: 70, 1024: 24}
    for V in (33, 64, 65, 96, 392, 1024):
        rng = np.random.default_rng(1000 + V)
        out, cases = {}, []
        for T in (1, 7) + ((long_T[V],) if V in long_T else ()):
            L = (rng.standard_normal((1, T, V)) * 3).astype(np.float32)
            g64, l64, g32 = ref_loss_grad(ref, L, 0.3, True, True, 0.0)
            _store(out, cases, f"canon_V{V}_T{T}", L, g64, l64, g32, [2.5, 0.3, 1.0, 1.0, 0.0])
        out["cases"] = np.array(cases)
        np.savez_compressed(os.path.join(HERE, f"g10_vocab_loss_v{V}.npz"), **out)
        print("g10", V, {c: float(out[f"{c}/ref_f32_relerr"]) for c in cases})
    # V = 96, T = 49: the hyper-parameter corners of g1 and exact argmax ties
    V, T = 96, 49
    rng = np.random.default_rng(1096)
    # (name, em, reweight, non_blank, div, blank_shift)
    specs = [("allblank", 0.3, True, True, 0.0, 50.0), ("em1", 1.0, False, True, 0.0, 0.0),
             ("em0", 0.0, True, False, 0.0, 0.0), ("noblankmask", 0.5, False, False, 0.0, 0.0),
             ("div", 0.3, True, True, 0.4, 0.0), ("ties", 0.3, True, True, 0.0, 0.0)]
    out, cases = {}, []
    for name, em, rw, nb, div, shift in specs:
        L = (rng.standard_normal((1, T, V)) * 3).astype(np.float32)
        L[..., 0] += shift
        if name == "ties":
            for t in range(T):
                top = np.float32(L[0, t].max() + 1.0)
                if t % 3 == 0:      # blank ties with a later class: the first maximum (blank) wins
                    L[0, t, 0] = L[0, t, 70] = top
                elif t % 3 == 1:    # two non-blank classes in different 64-class chunks tie
                    L[0, t, 5] = L[0, t, 80] = top
        g64, l64, g32 = ref_loss_grad(ref, L, em, rw, nb, div)
        _store(out, cases, f"{name}_V{V}_T{T}", L, g64, l64, g32, [2.5, em, float(rw), float(nb), div])
    out["cases"] = np.array(cases)
    np.savez_compressed(os.path.join(HERE, "g10_vocab_loss_v96_cases.npz"), **out)
    print("g10 cases", {c: float(out[f"{c}/ref_f32_relerr"]) for c in cases})


def g11(ref):
    steps, lr = 4, 5e-4
    for vname, preset, V in (("group_v41", "tiny-group", 41), ("layer_v392", "tiny-layer", 392)):
        cfg = get_config(preset)
        cfg["vocab_size"] = V
        sd = synth_weights(cfg)
        hp = dict(lr=lr, train_feature=True, bias_only=False, em=0.3, rw=True, nb=True, temp=2.5, div=0.0)
        for j, n in enumerate((8000, 12345)):
            out = {"weights_sha256": np.array(mg.weights_digest(sd)), "hp_json": np.array(repr(hp)),
                   "vocab_size": np.array(V), "steps": np.array(steps)}
            x = mg.wave(n, 70 + j)
            logits, final, names = mg.run_ref_suta(ref, cfg, sd, x, steps, **hp)
            out["x"] = x
            out["logits"] = np.stack([logits[i] for i in range(steps + 1)])
            for k, v in final.items():
                out[f"final/{k}"] = v
            out["entries"] = np.array(names)
            np.savez_compressed(os.path.join(HERE, f"g11_vocab_tiny_{vname}_N{n}.npz"), **out)
        print("g11", vname, "done")


def g12(ref):
    """A 96-token vocabulary with multi-character tokens and <pad> in the middle, decoded by HF."""
    from transformers import Wav2Vec2CTCTokenizer
    singles = [chr(c) for c in range(ord("a"), ord("z") + 1)] + list("äöüßéèñçøå'-")
    multi = ["ch", "sch", "th", "ng", "aa", "ee", "oo", "qu", "sz", "ts", "dʒ", "tʃ", "aɪ", "aʊ", "ɔɪ", "eɪ"]
    toks = singles + multi
    toks += [f"x{i}" for i in range(96 - 5 - len(toks))]
    rng = np.random.default_rng(12)
    rng.shuffle(toks)
    # specials: unk first, the delimiter and bos/eos inside, <pad> at id 17 (not 0, not the last)
    order = ["<unk>"] + toks[:3] + ["|"] + toks[3:15] + ["<pad>"] + toks[15:40] + ["<s>"] + toks[40:60] + ["</s>"] + toks[60:]
    assert len(order) == 96 and len(set(order)) == 96 and order[17] == "<pad>"
    vocab = {t: i for i, t in enumerate(order)}
    vpath = os.path.join(HERE, "g12_vocab96.json")
    with open(vpath, "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    tok = Wav2Vec2CTCTokenizer(vpath)
    assert tok.pad_token_id == 17
    cases = []
    for i in range(100):
        T = int(rng.integers(0, 60))
        p_blank = rng.uniform(0.2, 0.9)
        ids = [17 if rng.uniform() < p_blank else int(rng.integers(0, 96)) for _ in range(T)]
        if i % 7 == 0:  # long repeats and delimiter runs
            ids = [int(v) for v in np.repeat(rng.choice([0, 4, 17, 5, 30, 43, 64], size=max(1, T // 4)), 4)]
        cases.append({"ids": ids, "text": tok.batch_decode([ids])[0] if ids else tok.decode([])})
    with open(os.path.join(HERE, "g12_ctc_decode_vocab96.json"), "w", encoding="utf-8") as f:
        json.dump(cases, f, ensure_ascii=False)
    print("g12 done")


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref = mg.import_reference()
    for w in sys.argv[1:] or ["g10", "g11", "g12"]:
        globals()[w](ref)
