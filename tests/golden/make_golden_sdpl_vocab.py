"""Golden vectors for the SDPL pseudo-label objective on vocabularies other than the 32 letters, from the
REFERENCE's own main_SDPL.forward_and_adapt (main_SDPL.py:143-209) and a real Wav2Vec2CTCTokenizer.

Build container only (it reads the reference checkout through make_golden.py, whose helpers it imports):
    python tests/golden/make_golden_sdpl_vocab.py

The reference opens the vocab.json of its working directory; here it is handed the fixture vocabulary both as
`vocab` and as the processor's tokenizer: the one consistent reading for a checkpoint that is not the 960h one.

  g13_sdpl_vocab<V>.json       fixture vocab.json files, <pad> at id 0:
                                 33, 41  the 32 letters plus single characters (41: and "TH", "CH")
                                 96      single characters, multi-character tokens whose characters are all tokens
                                         (ch, sch, th, ...), four with a character that is no token, <s>, </s>,
                                         <unk>, the delimiter '|' at id 9
                                 392, 1024  single characters from Latin-1 to CJK
  g13_sdpl_loss_v<V>.npz       loss + dL/dlogits at T = 1 and 7 (pl 1 and 0.5), and at 96 the corner cases: all
  g13_sdpl_loss_v<V>_long.npz  blank (U = 0), leading / trailing delimiter runs, adjacent equal labels made by an
                               expansion ("c" then "ch"), a row-maximum tie across two 64-class chunks; _long: one
                               longer T (50 at 96, 30 at 392, 23 at 1024, 40 at 33).  Per case: fp32 logits, the fp64
                               gradient and loss, the reference's fp32 gradient, the target ids the reference handed
                               to nn.CTCLoss, hp = [temp, em_coef, reweight, non_blank, pl_coef].
  g14_sdpl_vocab_tiny_<variant>_N<n>.npz  tiny-config episodic SDPL (main_SDPL.py:327-349), 5 steps, a file per
                               length (8000 and 5000 samples): tiny-group at vocab_size 41 (lr 1e-4), tiny-layer
                               at 392 (lr 5e-4): logits and the reference's targets after every step, the final
                               trainable tensors, and
                               f64_same_target: per step whether the reference's own fp64 run built the same
                               pseudo label (the generator insists on all of them).
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

from suta_amd.config import get_config  # noqa: E402
from suta_amd.decode import (KIND_FAIL, KIND_NORMAL, VOCAB, CTCVocab, pseudo_label_table,  # noqa: E402
                             pseudo_label_target)
from suta_amd.weights import synth_weights  # noqa: E402

MAX_BYTES = os.path.getsize(os.path.join(HERE, "g10_vocab_loss_v1024.npz"))


def wide_chars(n, skip=()):
    out = []
    for lo, hi in ((0x00C0, 0x0250), (0x0391, 0x03CA), (0x0410, 0x0450), (0x3041, 0x3097), (0x30A1, 0x30FB),
                   (0x4E00, 0x5200)):
        for c in range(lo, hi):
            ch = chr(c)
            if ch.isalpha() and not ch.isspace() and ch not in skip and len(out) < n:
                out.append(ch)
    assert len(out) == n and len(set(out)) == n
    return out


def fixture_vocabs():
    v = {33: VOCAB + ["-"], 41: VOCAB + list("0123456") + ["TH", "CH"]}
    singles = [chr(c) for c in range(ord("a"), ord("z") + 1)] + list("äöüßéèñçøå'-")
    multi = ["ch", "sch", "th", "ng", "aa", "ee", "oo", "qu", "sz", "ts"]
    broken = ["dʒ", "tʃ", "aɪ", "ɔɪ"]
    rest = singles + multi + broken + ["<s>", "</s>", "<unk>"]
    rest += wide_chars(96 - 2 - len(rest), skip=set(singles))
    rng = np.random.default_rng(13)
    rng.shuffle(rest)
    v[96] = ["<pad>"] + rest[:8] + ["|"] + rest[8:]
    for V in (392, 1024):
        v[V] = ["<pad>", "<s>", "</s>", "<unk>", "|"] + wide_chars(V - 5)
    for V, toks in v.items():
        assert len(toks) == V and len(set(toks)) == V and toks[0] == "<pad>", V
    return v


def write_vocab(V, toks):
    path = os.path.join(HERE, f"g13_sdpl_vocab{V}.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({t: i for i, t in enumerate(toks)}, f, ensure_ascii=False)
    return path


def processor_for(path):
    from transformers import Wav2Vec2CTCTokenizer, Wav2Vec2FeatureExtractor, Wav2Vec2Processor
    fe = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True,
                                  return_attention_mask=False)
    return Wav2Vec2Processor(feature_extractor=fe, tokenizer=Wav2Vec2CTCTokenizer(path))


@contextlib.contextmanager
def recorded_targets(rec):
    """Record the target tensor the reference hands to nn.CTCLoss (main_SDPL.py:207)."""
    orig = torch.nn.CTCLoss.forward

    def fwd(self, log_probs, targets, input_lengths, target_lengths):
        rec.append(targets.detach().numpy().astype(np.int32).copy())
        return orig(self, log_probs, targets, input_lengths, target_lengths)
    torch.nn.CTCLoss.forward = fwd
    try:
        yield
    finally:
        torch.nn.CTCLoss.forward = orig


def ref_loss_grad(sdpl, L, hp, vocab, proc):
    """{dtype: (grad, loss)}, target of the reference objective at logits L (1, T, V)."""
    temp, em, rw, nb, pl = hp
    res, targets = {}, []
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
            with recorded_targets(targets):
                opt = torch.optim.SGD([fake.L], lr=1.0)
                sdpl.forward_and_adapt(None, fake, opt, em, bool(rw), temp, bool(nb), None, 0, True, pl, vocab, proc)
        finally:
            torch.Tensor.backward = orig
        res[dt] = (grads[0][0].numpy(), losses[0].item())
    assert np.array_equal(targets[0], targets[1])
    return res, targets[0]


def path_logits(rng, V, path):
    """Random logits whose greedy path is `path` (+40 on the chosen class of every frame)."""
    L = (rng.standard_normal((1, len(path), V)) * 3).astype(np.float32)
    for t, i in enumerate(path):
        L[0, t, i] += 40.0
    return L


def random_path(rng, tab, T, p_blank=0.45):
    """A greedy path over non-failing tokens whose expanded target still has a CTC alignment in T frames."""
    ok = [i for i, k in enumerate(tab.kinds) if k != KIND_FAIL and i != 0]
    single = [i for i in ok if tab.kinds[i] != KIND_NORMAL or tab.offsets[i + 1] - tab.offsets[i] == 1]
    for _ in range(1000):
        path = [0 if rng.uniform() < p_blank else int(rng.choice(ok if rng.uniform() < 0.3 else single))
                for _ in range(T)]
        tg = pseudo_label_target(path, tab)
        if tg and len(tg) + sum(a == b for a, b in zip(tg, tg[1:])) <= T:
            return path
    raise RuntimeError("no feasible path")


def g13(sdpl, vocabs):
    long_T = {33: 40, 96: 50, 392: 30, 1024: 23}  # 23: the file stays within the size of g10_vocab_loss_v1024.npz
    for V in (33, 96, 392, 1024):
        toks = vocabs[V]
        vpath = write_vocab(V, toks)
        proc = processor_for(vpath)
        vocab = json.load(open(vpath, encoding="utf-8"))
        tab = pseudo_label_table(CTCVocab(toks))
        idx = {t: i for i, t in enumerate(toks)}
        rng = np.random.default_rng(1300 + V)
        specs = []  # (name, logits, hp); pl 1 runs without the blank mask: 0 * the SUTA loss stays finite
        for T, pl in ((1, 1.0), (7, 1.0), (7, 0.5)):
            specs.append((f"pl{pl:g}_V{V}_T{T}", path_logits(rng, V, random_path(rng, tab, T)),
                          [2.5, 1.0, 0.0, 0.0, pl] if pl == 1.0 else [2.5, 0.3, 1.0, 1.0, pl]))
        if V == 96:
            T = 12
            bl, d = 0, idx["|"]
            L = (rng.standard_normal((1, T, V)) * 3).astype(np.float32)
            L[..., 0] += 60.0
            specs.append((f"allblank_V{V}_T{T}", L, [2.5, 1.0, 0.0, 0.0, 1.0]))
            a, b, c, ch, sch = idx["a"], idx["b"], idx["c"], idx["ch"], idx["sch"]
            specs.append((f"delims_V{V}_T{T}", path_logits(rng, V, [d, d, bl, d, a, d, bl, d, b, b, d, d]),
                          [2.5, 1.0, 0.0, 0.0, 1.0]))
            # "c" then "ch" -> c c h: the expansion makes adjacent equal labels (a blank is needed between them);
            # "sch" then "ch" -> s c h c h
            specs.append((f"adjacent_V{V}_T{T}", path_logits(rng, V, [c, ch, bl, bl, a, bl, sch, ch, bl, bl, bl, b]),
                          [2.5, 0.3, 1.0, 1.0, 0.5]))
            # exact ties of the row maximum between a class of chunk 0 and one of chunk 1: the first wins
            lo = min(a, b, c)
            hi = max(i for i in range(64, V) if tab.kinds[i] == KIND_NORMAL)
            L = path_logits(rng, V, [bl, lo, bl, lo, a, bl, b, bl, bl, lo, bl, c])
            for t in (1, 3, 9):
                L[0, t, hi] = L[0, t, lo]
            L[0, 0, hi] = L[0, 0, 0]          # blank ties with a later class: blank wins
            assert lo < 64 <= hi
            specs.append((f"ties_V{V}_T{T}", L, [2.5, 1.0, 0.0, 0.0, 1.0]))
        groups = {"": specs, "_long": [(f"pl1_V{V}_T{long_T[V]}",
                                        path_logits(rng, V, random_path(rng, tab, long_T[V])),
                                        [2.5, 1.0, 0.0, 0.0, 1.0])]}
        for suffix, group in groups.items():
            out, cases = {}, []
            for name, L, hp in group:
                res, target = ref_loss_grad(sdpl, L, hp, vocab, proc)
                g64, l64 = res[torch.float64]
                g32, l32 = res[torch.float32]
                assert np.isfinite(g64).all() and np.isfinite(l64), name
                assert target.tolist() == pseudo_label_target(L[0].argmax(-1), tab), name
                out[f"{name}/logits"] = L[0]
                out[f"{name}/grad_f64"] = g64
                out[f"{name}/loss_f64"] = np.array(l64)
                out[f"{name}/grad_f32"] = g32
                out[f"{name}/target"] = target
                out[f"{name}/hp"] = np.array(hp)
                cases.append(name)
                print("g13", name, "U", len(target), "loss", l64, "own", float(np.abs(g32 - g64).max()))
            out["cases"] = np.array(cases)
            out["vocab_size"] = np.array(V)
            fn = os.path.join(HERE, f"g13_sdpl_loss_v{V}{suffix}.npz")
            np.savez_compressed(fn, **out)
            assert os.path.getsize(fn) <= MAX_BYTES, (fn, os.path.getsize(fn))


def g14(sdpl, vocabs):
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
    steps = 5
    for vname, preset, V, lr in (("group_v41", "tiny-group", 41, 1e-4), ("layer_v392", "tiny-layer", 392, 5e-4)):
        toks = vocabs[V]
        vpath = write_vocab(V, toks)
        proc = processor_for(vpath)
        vocab = json.load(open(vpath, encoding="utf-8"))
        tab = pseudo_label_table(CTCVocab(toks))
        cfg = get_config(preset)
        cfg["vocab_size"] = V
        sd = synth_weights(cfg, blank_bias=0.0)
        fail = [i for i, k in enumerate(tab.kinds) if k == KIND_FAIL]
        sd["lm_head.bias"][fail] -= 30.0  # keep lookup-failure ids off the greedy path (reference KeyError)
        head = {"weights_sha256": np.array(mg.weights_digest(sd)), "lr": np.array(lr), "vocab_size": np.array(V),
               "steps": np.array(steps), "fail_ids": np.array(fail, np.int32)}

        def run(x, dt):
            torch.manual_seed(0)
            model = Wav2Vec2ForCTC(Wav2Vec2Config(**cfg)).eval()
            model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            model = sdpl.configure_model(model.to(dt))
            with contextlib.redirect_stdout(io.StringIO()):
                params, names = sdpl.collect_params(model, False, True)
                opt, sch = sdpl.setup_optimizer(params, "Adam", lr, scheduler=None)
            xt = torch.from_numpy(x).to(dt)[None]
            logits, targets = [], []
            with torch.no_grad():
                logits.append(model(xt).logits[0].numpy().copy())
            with recorded_targets(targets):
                for _ in range(steps):
                    o = sdpl.forward_and_adapt(xt, model, opt, 1.0, False, 2.5, True, sch, div_coef=0,
                                               repeat_inference=True, pl_coef=1., vocab=vocab, processor=proc)
                    logits.append(o[0].detach().numpy().copy())
            sdf = model.state_dict()
            return logits, targets, {k: sdf[k].numpy().copy() for k in dict.fromkeys(names)}

        for j, n in enumerate((8000, 5000)):
            for seed in range(130 + 10 * j, 140 + 10 * j):  # the first wave whose fp32 and fp64 runs share every target
                x = mg.wave(n, seed)
                l32, t32, final = run(x, torch.float32)
                l64, t64, _ = run(x, torch.float64)
                same = [a.tolist() == b.tolist() for a, b in zip(t32, t64)]
                finite = all(np.isfinite(l).all() for l in l32)
                print("g14", vname, n, "seed", seed, "same", same, "U", [len(t) for t in t32], "finite", finite)
                if all(same) and finite:
                    break
            else:
                raise RuntimeError("no wave with matching fp32 / fp64 pseudo labels")
            res = dict(head)
            for i, t in enumerate(t32):
                assert t.tolist() == pseudo_label_target(l32[i].argmax(-1), tab)
                res[f"target{i}"] = t
            res["x"] = x
            res["wave_seed"] = np.array(seed)
            res["logits"] = np.stack(l32)
            res["f64_same_target"] = np.array(same)
            res["f64_max_logit_dev"] = np.array(max(float(np.abs(a - b).max()) for a, b in zip(l32, l64)))
            for k, v in final.items():
                res[f"final/{k}"] = v
            fn = os.path.join(HERE, f"g14_sdpl_vocab_tiny_{vname}_N{n}.npz")
            np.savez_compressed(fn, **res)
            assert os.path.getsize(fn) <= MAX_BYTES, (fn, os.path.getsize(fn))
            print("g14", vname, n, "done", os.path.getsize(fn))


if __name__ == "__main__":
    torch.set_num_threads(8)
    sdpl = mg.import_reference_sdpl()
    vocabs = fixture_vocabs()
    for V, toks in vocabs.items():
        write_vocab(V, toks)
    for w in sys.argv[1:] or ["g13", "g14"]:
        globals()[w](sdpl, vocabs)
