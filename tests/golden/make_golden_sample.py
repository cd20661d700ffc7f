#!/usr/bin/env python3
"""Golden rows of the byte sampler, produced by the REFERENCE's own code on CPU: `sample_next` of
scripts/stream_generate_fast.py:146-170 and `generate` of fft_lm/train_fixed_full.py:621-704.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sample.py

`generate` gets a stub model that returns preset logits for the last position, and in both functions torch.multinomial
is replaced by a recorder that stores the `probs` it is handed and returns a preset id: what is recorded is the
distribution the reference draws from, after all its penalties, bans, nucleus and top-k.

Y01_sample_rows.npz holds, per case `c` of `cases`: c.logits (R, 256) fp32, c.recent int64 (the window the reference
penalises: its last repetition_window ids), c.u (R) fp32, c.probs (R, 256) fp32 as recorded, c.settings (the keyword
arguments of functional.sample_bytes as JSON).  Only rows comparable by the margin rule of tests/sample_common.py are
stored, and the generator FAILS unless the reference's rows have exactly the restatement's support and lie within
1e-5 of it.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                     # noqa: E402  (puts the reference on sys.path)
from make_golden import REF                                  # noqa: E402
import sample_common as sc                                   # noqa: E402

from fft_lm import train_fixed_full as tff                   # noqa: E402

_spec = importlib.util.spec_from_file_location("stream_generate_fast", os.path.join(REF, "scripts", "stream_generate_fast.py"))
sgf = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sgf)

ROWS = 8


class Recorder:
    """Stands in for torch.multinomial: keeps the distribution, returns the preset id."""

    def __init__(self):
        self.probs = []

    def __call__(self, probs, n, **kw):
        assert n == 1 and probs.dim() == 1
        self.probs.append(probs.detach().clone())
        return torch.tensor([65])


class StubLM:
    """model(x, cutoff=...) -> (1, T, 256) logits whose last position is the preset row."""

    def __init__(self, row):
        self.row = row

    def eval(self):
        return self

    def __call__(self, x, cutoff=None):
        out = torch.zeros(1, x.shape[1], 256)
        out[0, -1] = self.row
        return out


def ascii_window(n, seed, run=0):
    """n ids below 128 (a prompt string encodes to exactly these bytes); the last `run` are one byte."""
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([32, 10, 13, 46] + list(range(97, 123))), n).astype(np.int64)
    if run:
        w[n - run:] = 101
    return w


def via_generate(logits, window, **cfg_kw):
    """One call of the reference's generate per row, max_new = 1; returns (recorded probs, settings, recent)."""
    cfg = tff.TrainConfig(max_new=1, seq_len=1024, device="cpu", **cfg_kw)
    rec, real = Recorder(), torch.multinomial
    torch.multinomial = rec
    try:
        for row in logits:
            tff.generate(StubLM(torch.from_numpy(row)), bytes(window.tolist()).decode("ascii"), cfg, "cpu")
    finally:
        torch.multinomial = real
    settings = dict(temperature=cfg.temperature, top_p=cfg.top_p, top_k=cfg.top_k,
                    repetition_penalty=cfg.repetition_penalty, presence_penalty=cfg.presence_penalty,
                    frequency_penalty=cfg.frequency_penalty, ascii_only=cfg.ascii_only, ban_cr=cfg.ban_cr,
                    max_run_length=cfg.max_run_length)
    return torch.stack(rec.probs).numpy(), settings, window[-cfg.repetition_window:]


def via_sample_next(logits, window, temperature, top_p, top_k, rep):
    rec, real = Recorder(), torch.multinomial
    torch.multinomial = rec
    try:
        for row in logits:
            sgf.sample_next(torch.from_numpy(row), temperature, top_p, top_k, rep, window.tolist())
    finally:
        torch.multinomial = real
    settings = dict(temperature=temperature, top_p=top_p, top_k=top_k, repetition_penalty=rep)
    return torch.stack(rec.probs).numpy(), settings, window[-256:]


def cases():
    lg = lambda seed, scale=3.0: sc.make_rows(ROWS, seed, scale)
    e = np.zeros(0, np.int64)
    yield "defaults", lg(1), lambda l: via_generate(l, ascii_window(256, 11))
    yield "presence_frequency", lg(2), lambda l: via_generate(l, ascii_window(256, 12), presence_penalty=0.3,
                                                              frequency_penalty=0.05)
    yield "topk5_narrow_nucleus", lg(3), lambda l: via_sample_next(l, ascii_window(64, 13), 0.8, 0.5, 5, 1.25)
    yield "topk5_wide_nucleus", sc.make_rows(4 * ROWS, 4), lambda l: via_sample_next(l, ascii_window(64, 14), 1.0, 0.9, 5, 1.25)
    yield "run_of_6", lg(5), lambda l: via_generate(l, ascii_window(256, 15, run=6))
    yield "n_recent_0", lg(6), lambda l: via_sample_next(l, e, 0.8, 0.9, 0, 1.25)
    yield "n_recent_1", lg(7), lambda l: via_sample_next(l, np.array([101], np.int64), 0.8, 0.9, 0, 1.25)
    yield "n_recent_300", lg(8), lambda l: via_generate(l, ascii_window(300, 16), repetition_window=512)
    yield "top_p_1", lg(9), lambda l: via_sample_next(l, ascii_window(64, 17), 0.8, 1.0, 0, 1.25)
    yield "top_p_1_generate", lg(10), lambda l: via_generate(l, ascii_window(256, 18), top_p=1.0)


def main():
    rec, names = {}, []
    for name, (logits, u), run in cases():
        probs, settings, recent = run(logits)
        assert probs.dtype == np.float32 and probs.shape == logits.shape
        ids, p64, ok = sc.restate(logits, recent, u, **settings)
        if name.startswith("topk5"):                                     # by what the nucleus alone keeps
            kept = (sc.restate(logits, recent, u, **dict(settings, top_k=0))[1] > 0).sum(axis=1)
            ok &= (kept < 5) if "narrow" in name else (kept > 5)
            assert ((probs > 0).sum(axis=1) == np.minimum(kept, 5))[ok].all(), name
        assert ok.sum() >= 4, (name, sc.share(ok))
        logits, u, probs, p64 = logits[ok], u[ok], probs[ok], p64[ok]
        assert np.array_equal(probs > 0, p64 > 0), name                  # the reference and the definition agree ...
        err = float(np.abs(probs - p64).max())
        assert err <= 1e-5, (name, err)                                  # ... to the tests' tolerance
        if name == "run_of_6":
            assert (probs[:, 101] == 0).all()
        print(f"{name}: {int(ok.sum())} of {len(ok)} rows, max |reference - restatement| = {err:.2e}")
        names.append(name)
        rec.update({name + ".logits": logits, name + ".recent": np.asarray(recent, np.int64), name + ".u": u,
                    name + ".probs": probs, name + ".settings": np.array(json.dumps(settings))})
    rec["cases"] = np.array(names)
    mg.save("Y01_sample_rows", rec)


if __name__ == "__main__":
    main()
