#!/usr/bin/env python3
"""Golden vectors of the training loop's host logic, produced by the REFERENCE on CPU: the schedule functions and
TrainConfig of fft_lm/train_fixed_full.py (:34-105, :129-147, :208-424).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_training.py

L01: recorded results of the reference's own schedule functions over grids of their arguments -- sawtooth_lr for every
(epoch, step) of an 8-epoch run at steps_per_epoch=5, with and without cutoff_raised; the cutoff functions over epochs
0-120, bin counts {65, 513, 1025} and loss histories that plateau, improve and are too short; make_val_starts for two
seeds; conv_freq_bins for the (seq_len, kernel_len) pairs the scripts use -- and the field names and default values of
its TrainConfig.
"""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                     # noqa: E402  (puts the reference on sys.path)

from fft_lm import train_fixed_full as ref                   # noqa: E402

BINS = (65, 513, 1025)
HISTORIES = {
    "plateau": [2.0 + 1e-4 * ((i * 7) % 5) for i in range(60)],
    "improve": [3.0 - 0.02 * i for i in range(60)],
    "short": [2.0] * 10,
}
PAIRS = [(1024, 128), (512, 128), (256, 64), (64, 8), (1024, 1), (100, 16), (2048, 128)]


def schedules_case(name):
    rec = {}
    cfg = ref.TrainConfig(steps_per_epoch=5, epochs=8)
    for raised in (False, True):
        rec[f"sawtooth.raised{int(raised)}"] = np.array(
            [[ref.sawtooth_lr(e * 5 + s, e, cfg, cutoff_raised=raised) for s in range(5)] for e in range(8)], np.float64)
    stages = [ref.lr_stage_params(e, cfg) for e in range(8)]
    rec["stage.names"] = np.array([s[0] for s in stages])
    rec["stage.mults"] = np.array([s[1:] for s in stages], np.float64)
    dcfg = ref.TrainConfig()
    rec["bins"] = np.array(BINS)
    rec["curriculum"] = np.array([[ref.curriculum_cutoff(e, dcfg, b) for e in range(121)] for b in BINS])
    rec["jpeg"] = np.array([[ref.jpeg_cutoff(e, dcfg, b) for e in range(121)] for b in BINS])
    rows = []
    for hi, (hname, hist) in enumerate(HISTORIES.items()):
        rec["history." + hname] = np.array(hist, np.float64)
        for epoch in (0, 1, 5):
            for cur in (128, 512, 1025):
                for b in BINS:
                    new, raised = ref.adaptive_cutoff(epoch, cur, list(hist), b)
                    rows.append((hi, epoch, cur, b, new, int(raised)))
    rec["adaptive"] = np.array(rows)                          # history index, epoch, cutoff, bins -> new cutoff, raised
    rec["adaptive.histories"] = np.array(list(HISTORIES))
    rows = []
    for cur in (128, 512, 1025):
        for loss in (1.0, 1.995, 2.5):
            for b in BINS:
                for counter in (0, 48, 49, 60):
                    new, raised, best, cnt = ref.plateau_cutoff(cur, loss, b, 2.0, counter)
                    rows.append((cur, loss, b, counter, new, int(raised), best, cnt))
    rec["plateau"] = np.array(rows, np.float64)               # cutoff, loss, bins, counter -> cutoff, raised, best, counter
    rec["val_starts.args"] = np.array([[100000, 1024, 16, 1338], [5000, 512, 16, 7]])
    for i, a in enumerate(rec["val_starts.args"]):
        rec[f"val_starts.{i}"] = ref.make_val_starts(*(int(v) for v in a))
    rec["conv_bins.pairs"] = np.array(PAIRS)
    rec["conv_bins"] = np.array([ref.conv_freq_bins(s, k) for s, k in PAIRS])
    fields = dataclasses.fields(ref.TrainConfig)
    rec["config.names"] = np.array([f.name for f in fields])
    rec["config.defaults"] = np.array([repr(getattr(dcfg, f.name)) for f in fields])
    rec["config.types"] = np.array([type(getattr(dcfg, f.name)).__name__ for f in fields])
    mg.save(name, rec)


if __name__ == "__main__":
    schedules_case("L01_schedules")
