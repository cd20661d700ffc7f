#!/usr/bin/env python3
"""Golden vectors of what the trainer runs at the end of an epoch, produced by the REFERENCE on CPU: parroting_score and
eval_loss of fft_lm/train_fixed_full.py (:185-205, :150-182) and the load_state_flexible of its main() (:824-850).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py

V01_parroting.npz: a 6 KiB word corpus (eval_common.text_corpus) and, per generation `g` of `names`: g.gen (its bytes),
g.picks (what the reference's np.random.default_rng(123).choice returned, recorded by wrapping default_rng; empty where
it returns early) and g.score.  Generations of 64, 65, 100, 464 and 2000 bytes with the default TrainConfig (so
snippets of 64 bytes every 16, at most 64 of them), one copied wholesale from the corpus and one half copied.
V02_eval_loss.npz: per geometry of eval_common.GEOMETRIES the state dict of a reference FixedSpectralLM (d_model 32, 2
layers, gate_ctx.weight and a std-0.05 kernel away from their defaults so that the loss depends on the convolution), the
starts of make_val_starts over an 8 KiB corpus, and the reference's eval_loss after torch.manual_seed(seed) at
batch_size 2, val_batches 2 -- for cutoff None and one cutoff below the bin count -- from the model in float64
(`loss64.*`, what the tests compare with) and in fp32 (`loss32.*`), with `ref_err_*` = their relative distance, which must
stay within a quarter of the tests' tolerance.
V03_flexible.npz: the (resized, skipped) lists of the reference's load_state_flexible when a state dict saved at
seq_len 48 / kernel_len 16 is loaded into a model of seq_len 112 / kernel_len 24, with one unknown key.
"""
import ast
import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                     # noqa: E402  (puts the reference on sys.path)
from make_golden import REF, SEED                            # noqa: E402
import eval_common as ec                                     # noqa: E402
from conftest import TOL_ACT, rel_err                        # noqa: E402

from fft_lm import train_fixed_full as ref                   # noqa: E402

GEOMETRY = {"conv": (448, 65, 100), "filter": (48, 16, 20)}   # seq_len, kernel_len, cutoff (257 and 33 bins)


def parroting_case(name):
    corpus = ec.text_corpus(6144, SEED)
    gens = {
        "short64": ec.novel_bytes(64, 1),
        "edge65": ec.novel_bytes(65, 2),
        "copied100": corpus[1000:1100],
        "novel464": ec.novel_bytes(464, 3),
        "mixed2000": b"".join(corpus[300 * i:300 * i + 100] + ec.novel_bytes(100, 10 + i) for i in range(10)),
        "copied464": corpus[2000:2464],
        "half464": corpus[4000:4232] + ec.novel_bytes(232, 4),
    }
    cfg = ref.TrainConfig()
    rec = {"corpus": np.frombuffer(corpus, np.uint8), "names": np.array(list(gens))}
    real_rng = np.random.default_rng
    for g, gen in gens.items():
        drawn = []

        class Wrapped:
            def __init__(self, seed):
                assert seed == 123
                self.rng = real_rng(seed)

            def choice(self, *a, **k):
                drawn.append(np.asarray(self.rng.choice(*a, **k)))
                return drawn[-1]

        np.random.default_rng = Wrapped
        try:
            score = ref.parroting_score(corpus, gen, cfg)
        finally:
            np.random.default_rng = real_rng
        assert len(drawn) <= 1
        rec[g + ".gen"] = np.frombuffer(gen, np.uint8)
        rec[g + ".picks"] = drawn[0].astype(np.int64) if drawn else np.empty(0, np.int64)
        rec[g + ".score"] = np.float64(score)
    assert rec["mixed2000.picks"].size == 64 < len(range(32, 2000 - 64, 16))       # choice really subsamples
    assert rec["copied464.score"] == 1.0 and rec["novel464.score"] == 0.0 and 0.0 < rec["half464.score"] < 1.0
    assert 0.0 < rec["mixed2000.score"] < 1.0 and rec["copied100.picks"].size == 1 and rec["edge65.picks"].size == 0
    mg.save(name, rec)


def eval_loss_case(name, seed=4321):
    corpus = torch.from_numpy(np.frombuffer(ec.text_corpus(8192, SEED + 1), np.uint8).copy())
    rec = {"corpus": corpus, "seed": np.int64(seed), "d_model": np.int64(32), "n_layers": np.int64(2),
           "batch_size": np.int64(2), "val_batches": np.int64(2)}
    for geom, (seq_len, kernel_len, cutoff) in GEOMETRY.items():
        cfg = ref.TrainConfig(d_model=32, n_layers=2, seq_len=seq_len, kernel_len=kernel_len, batch_size=2,
                              val_batches=2, device="cpu")
        torch.manual_seed(SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            model = ref.FixedSpectralLM(cfg)
        with torch.no_grad():
            for blk in model.blocks:
                blk.kernel.normal_(0.0, 0.05)
                blk.gate_ctx.weight.normal_(0.0, 0.3)
                blk.gain.normal_(1.0, 0.2)
                blk.gate_freq_logits.normal_(1.0, 1.0)
        starts = ref.make_val_starts(int(corpus.numel()), seq_len, 16, seed + 1)
        model64 = copy.deepcopy(model).double()
        assert ref.conv_freq_bins(seq_len, kernel_len) > cutoff
        for cname, c in (("none", None), ("cut", cutoff)):
            torch.manual_seed(seed)
            l32 = ref.eval_loss(model, corpus, starts, cfg, c)
            torch.manual_seed(seed)
            l64 = ref.eval_loss(model64, corpus, starts, cfg, c)
            e = rel_err(np.float64(l32), np.float64(l64))
            assert e <= TOL_ACT / 4, (geom, cname, e)
            rec.update({f"{geom}.loss32.{cname}": np.float64(l32), f"{geom}.loss64.{cname}": np.float64(l64),
                        f"{geom}.ref_err_{cname}": np.float64(e)})
        assert abs(rec[f"{geom}.loss64.none"] - rec[f"{geom}.loss64.cut"]) > 1e-3      # the horizon matters
        rec.update({geom + ".seq_len": np.int64(seq_len), geom + ".kernel_len": np.int64(kernel_len),
                    geom + ".cutoff": np.int64(cutoff), geom + ".starts": starts})
        for k, v in model.state_dict().items():
            rec[f"{geom}.sd.{k}"] = v
    mg.save(name, rec)


def reference_load_state_flexible():
    """The reference's load_state_flexible is a closure of its main(): compile that one nested definition from the
    reference's source, in the reference module's namespace."""
    path = os.path.join(REF, "fft_lm", "train_fixed_full.py")
    tree = ast.parse(open(path).read())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    fn = next(n for n in ast.walk(main) if isinstance(n, ast.FunctionDef) and n.name == "load_state_flexible")
    ns = dict(vars(ref))
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["load_state_flexible"]


def flexible_case(name):
    load_state_flexible = reference_load_state_flexible()
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        old = ref.FixedSpectralLM(ref.TrainConfig(d_model=16, n_layers=2, seq_len=48, kernel_len=16))
        new = ref.FixedSpectralLM(ref.TrainConfig(d_model=16, n_layers=2, seq_len=112, kernel_len=24))
    state = dict(old.state_dict())
    state["not.in.the.model"] = torch.zeros(3)
    resized, skipped = load_state_flexible(new, state)
    assert len(resized) == 2 and len(skipped) == 2
    fmt = lambda rows: np.array([f"{k} {tuple(a)} {tuple(b)}" for k, a, b in rows])
    mg.save(name, {"resized": fmt(resized), "skipped": fmt(skipped), "old": np.array([16, 2, 48, 16]),
                   "new": np.array([16, 2, 112, 24]), "unknown_key": np.array("not.in.the.model")})


if __name__ == "__main__":
    parroting_case("V01_parroting")
    eval_loss_case("V02_eval_loss")
    flexible_case("V03_flexible")
