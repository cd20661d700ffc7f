"""The training-loop pieces of tensor_cuda_fft_amd.training without a GPU: TrainConfig and the schedules against the
reference's recorded results (L01, exactly), and sample_windows against the reference's slicing."""
import dataclasses

import numpy as np
import pytest
import torch

from conftest import load_golden

NAMES = ("TrainConfig", "conv_freq_bins", "jpeg_cutoff",
         "curriculum_cutoff", "adaptive_cutoff", "plateau_cutoff", "sawtooth_lr", "lr_stage_params", "make_val_starts",
         "sample_windows")


def pkg():
    import tensor_cuda_fft_amd
    return tensor_cuda_fft_amd


@pytest.fixture(scope="module")
def sched():
    return load_golden("L01_schedules")


def test_names_are_exported():
    p = pkg()
    for n in NAMES:
        assert n in p.__all__ and hasattr(p, n), n


# ---- schedules and config against the reference's recorded results --------------------------------------------------------
def test_train_config_has_the_reference_fields_and_defaults(sched):
    cfg = pkg().TrainConfig()
    fields = dataclasses.fields(cfg)
    assert [f.name for f in fields] == list(sched["config.names"])
    for name, default, tname in zip(sched["config.names"], sched["config.defaults"], sched["config.types"]):
        if name == "device":                                  # "cuda" where one is visible: the machine's, not the recorder's
            assert cfg.device == ("cuda" if torch.cuda.is_available() else "cpu")
            continue
        assert repr(getattr(cfg, name)) == default and type(getattr(cfg, name)).__name__ == tname, name


def test_fixed_spectral_lm_takes_a_train_config():
    p = pkg()
    cfg = p.TrainConfig(d_model=16, n_layers=1, seq_len=32, kernel_len=8)
    model = p.FixedSpectralLM(cfg)
    ref = p.FixedSpectralLM(p.LMConfig(d_model=16, n_layers=1, seq_len=32, kernel_len=8))
    assert sorted(model.state_dict()) == sorted(ref.state_dict())
    assert model(torch.zeros(2, 32, dtype=torch.long)).shape == (2, 32, 256)


def test_sawtooth_lr_and_stage_params_match_the_reference_exactly(sched):
    p = pkg()
    cfg = p.TrainConfig(steps_per_epoch=5, epochs=8)
    for raised in (False, True):
        got = np.array([[p.sawtooth_lr(e * 5 + s, e, cfg, cutoff_raised=raised) for s in range(5)] for e in range(8)])
        assert np.array_equal(got, sched[f"sawtooth.raised{int(raised)}"])
    stages = [p.lr_stage_params(e, cfg) for e in range(8)]
    assert [s[0] for s in stages] == list(sched["stage.names"])
    assert np.array_equal(np.array([s[1:] for s in stages]), sched["stage.mults"])
    assert all(isinstance(s[1], float) and isinstance(s[2], float) for s in stages)


def test_cutoff_schedules_match_the_reference_exactly(sched):
    p = pkg()
    cfg = p.TrainConfig()
    bins = [int(b) for b in sched["bins"]]
    assert np.array_equal(np.array([[p.curriculum_cutoff(e, cfg, b) for e in range(121)] for b in bins]), sched["curriculum"])
    assert np.array_equal(np.array([[p.jpeg_cutoff(e, cfg, b) for e in range(121)] for b in bins]), sched["jpeg"])
    hists = [list(sched["history." + str(h)]) for h in sched["adaptive.histories"]]
    assert [len(h) for h in hists] == [60, 60, 10]             # plateau, improve, too short
    seen = set()
    for hi, epoch, cur, b, new, raised in sched["adaptive"]:
        got = p.adaptive_cutoff(int(epoch), int(cur), hists[hi], int(b))
        assert got == (int(new), bool(raised)) and isinstance(got[1], bool)
        seen.add(bool(raised))
    assert seen == {False, True}
    seen = set()
    for cur, loss, b, counter, new, raised, best, cnt in sched["plateau"]:
        got = p.plateau_cutoff(int(cur), float(loss), int(b), 2.0, int(counter))
        assert got == (int(new), bool(raised), float(best), int(cnt))
        seen.add(bool(raised))
    assert seen == {False, True}


def test_val_starts_and_conv_bins_match_the_reference_exactly(sched):
    p = pkg()
    for i, a in enumerate(sched["val_starts.args"]):
        got = p.make_val_starts(*(int(v) for v in a))
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), sched[f"val_starts.{i}"])
    assert [p.conv_freq_bins(int(s), int(k)) for s, k in sched["conv_bins.pairs"]] == list(sched["conv_bins"])


def test_sample_windows_is_the_reference_slicing():
    p = pkg()
    torch.manual_seed(3)
    corpus = torch.randint(0, 256, (1000,), dtype=torch.uint8)
    T = 64
    starts = torch.tensor([0, 17, 1000 - (T + 1), 500])        # the first and the last admissible start among them
    x, y = p.sample_windows(corpus, starts, T)
    bx = torch.stack([corpus[s:s + T] for s in starts]).to(torch.long)
    by = torch.stack([corpus[s + 1:s + T + 1] for s in starts]).to(torch.long)
    assert x.dtype == y.dtype == torch.int64 and x.is_contiguous() and y.is_contiguous()
    assert torch.equal(x, bx) and torch.equal(y, by)
    with pytest.raises(IndexError):
        p.sample_windows(corpus, torch.tensor([1000 - T]), T)
    with pytest.raises(ValueError):
        p.sample_windows(corpus.view(10, 100), starts, T)
