"""The training loop pieces of the reference's trainer (fft_lm/train_fixed_full.py: TrainConfig :34-105, the cutoff and
learning-rate schedules :129-147 and :208-424, the window sampling of its loop :897-959), written against its behaviour:
a config with the same fields and defaults, the same schedule values, and the window sampling as one gather -- and what
the trainer runs at the end of every epoch (scripts/eval_ckpt.py runs the same on a saved model): load_corpus_as_u8
:115-126, eval_loss :150-182, parroting_score :185-205 on one native corpus scan (functional.find_snippets), the
checkpoint I/O of fft_lm/ckpt_io.py and the resume logic of main() (:824-893).  Out of scope: the CLIs and the optimizer
step.
"""
from __future__ import annotations

import hashlib
import math
import os
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from .functional import cross_entropy, find_snippets


@dataclass
class TrainConfig:
    """The reference's TrainConfig: same field names, same defaults (FixedSpectralLM reads the model fields, generate()
    the generation fields, the schedules below the rest)."""
    data_path: str = "tinystories_train.txt"
    # model
    vocab_size: int = 256
    d_model: int = 512
    n_layers: int = 6
    seq_len: int = 1024
    kernel_len: int = 128
    ffn_mult: int = 2
    frequency_native: bool = False
    use_fp32: bool = False
    bicameral: bool = False
    # optimisation
    batch_size: int = 8
    accum_steps: int = 1
    epochs: int = 200
    steps_per_epoch: int = 250
    lr: float = 2e-4
    weight_decay: float = 5e-4
    grad_clip: float = 1.0
    # frequency horizon
    jpeg_low: int = 128
    jpeg_mid: int = 512
    jpeg_high: int = 1024
    jpeg_transition: int = 32
    # generation
    temperature: float = 0.8
    top_p: float = 0.9
    top_k: int = 0
    repetition_penalty: float = 1.25
    repetition_window: int = 256
    max_run_length: int = 6
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    ban_cr: bool = True
    ascii_only: bool = True
    max_new: int = 400
    # run
    seed: int = 1337
    device: str = "cuda" if torch.cuda.is_available() else "cpu"
    amp: bool = True
    ckpt_path: str = "fixed_spectral_ckpt.pt"
    save_every_epochs: int = 5
    # validation
    val_windows: int = 2048
    val_batches: int = 20
    parroting_snip_len: int = 64
    parroting_stride: int = 16
    parroting_snips: int = 64
    log_every_steps: int = 50
    # learning-rate stages: cosine decay inside a stage, restart at its first step
    stage1_epochs: int = 1
    stage2_epochs: int = 3
    stage1_lr_mult: float = 1.0
    stage1_min_mult: float = 0.1
    stage2_lr_mult: float = 1.0
    stage2_min_mult: float = 0.1
    stage3_lr_mult: float = 1.0
    stage3_min_mult: float = 0.05


def conv_freq_bins(seq_len: int, kernel_len: int) -> int:
    """One-sided bin count of the causal convolution's transform: n_fft = the power of two that holds
    seq_len + kernel_len - 1 samples, n_fft / 2 + 1 bins."""
    n_fft = 1
    while n_fft < int(seq_len + kernel_len - 1):
        n_fft *= 2
    return n_fft // 2 + 1


def make_val_starts(n_bytes: int, seq_len: int, count: int, seed: int) -> torch.Tensor:
    """`count` window starts in [0, n_bytes - seq_len - 2), drawn from a CPU generator seeded with `seed`."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    return torch.randint(0, max(1, n_bytes - (seq_len + 1) - 1), (count,), generator=gen)


def jpeg_cutoff(epoch: int, cfg, freq_bins: int) -> int:
    """The four-step horizon by epoch: jpeg_low below 20, jpeg_mid below 50, jpeg_high below 100, then every bin."""
    for below, target in ((20, cfg.jpeg_low), (50, cfg.jpeg_mid), (100, cfg.jpeg_high)):
        if epoch < below:
            return int(min(target, freq_bins))
    return int(freq_bins)


def curriculum_cutoff(epoch: int, cfg, freq_bins: int) -> int:
    """The two-step horizon the trainer's loop uses: 128 bins for epochs 0-4, 512 from epoch 5 on, capped at freq_bins."""
    return int(min(128 if epoch < 5 else 512, freq_bins))


def _next_cutoff(current_cutoff: int, freq_bins: int) -> int:
    """The raise both plateau rules make: to 512 from below it, to every bin from there."""
    return min(512 if current_cutoff < 512 else freq_bins, freq_bins)


def adaptive_cutoff(epoch: int, current_cutoff: int, loss_history, freq_bins: int, *, min_epoch_before_raise: int = 1,
                    plateau_window: int = 50, plateau_threshold: float = 0.005) -> tuple:
    """(cutoff, raised): raise the horizon when the mean loss of the newer half of the last `plateau_window` steps
    improved on the older half by less than `plateau_threshold` (relative) -- never before `min_epoch_before_raise`,
    at full horizon, or with a shorter history."""
    if (epoch < min_epoch_before_raise or current_cutoff >= freq_bins or len(loss_history) < plateau_window
            or plateau_window < 2):
        return current_cutoff, False
    recent = loss_history[-plateau_window:]
    older, newer = recent[:plateau_window // 2], recent[plateau_window // 2:]
    mean_old, mean_new = sum(older) / len(older), sum(newer) / len(newer)
    gain = (mean_old - mean_new) / mean_old if mean_old > 0 else 0.0
    if gain >= plateau_threshold:
        return current_cutoff, False
    new = _next_cutoff(current_cutoff, freq_bins)
    return new, new > current_cutoff


def plateau_cutoff(current_cutoff: int, recent_loss: float, freq_bins: int, best_loss_at_cutoff: float,
                   steps_without_improvement: int, *, patience: int = 50, improvement_threshold: float = 0.01) -> tuple:
    """(cutoff, raised, best_loss, counter): count the steps on which `recent_loss` did not beat the best loss at this
    horizon by `improvement_threshold`; after `patience` of them raise the horizon and start over (best = inf)."""
    if current_cutoff >= freq_bins:
        return current_cutoff, False, best_loss_at_cutoff, steps_without_improvement
    if recent_loss < best_loss_at_cutoff - improvement_threshold:
        return current_cutoff, False, recent_loss, 0
    counter = steps_without_improvement + 1
    if counter >= patience:
        new = _next_cutoff(current_cutoff, freq_bins)
        if new > current_cutoff:
            return new, True, float("inf"), 0
    return current_cutoff, False, best_loss_at_cutoff, counter


def _lr_stage(epoch: int, cfg) -> tuple:
    """(name, first epoch, epochs, lr_mult, min_mult) of the stage `epoch` falls in"""
    e1 = int(cfg.stage1_epochs)
    e2 = e1 + int(cfg.stage2_epochs)
    if epoch < e1:
        return "stage1", 0, e1, cfg.stage1_lr_mult, cfg.stage1_min_mult
    if epoch < e2:
        return "stage2", e1, int(cfg.stage2_epochs), cfg.stage2_lr_mult, cfg.stage2_min_mult
    return "stage3", e2, int(cfg.epochs) - e2, cfg.stage3_lr_mult, cfg.stage3_min_mult


def lr_stage_params(epoch: int, cfg) -> tuple:
    """(stage name, lr_mult, min_mult) of `epoch`."""
    name, _, _, lr_mult, min_mult = _lr_stage(epoch, cfg)
    return name, float(lr_mult), float(min_mult)


def sawtooth_lr(global_step: int, epoch: int, cfg, *, cutoff_raised: bool = False) -> float:
    """Learning rate of optimizer step `global_step`: inside each stage a half cosine from lr * lr_mult down to
    lr * min_mult over the stage's steps, restarting at the stage's first step; `cutoff_raised` returns the stage's peak."""
    _, first_epoch, n_epochs, lr_mult, min_mult = _lr_stage(epoch, cfg)
    if cutoff_raised:
        return float(cfg.lr * lr_mult)
    per_epoch = int(cfg.steps_per_epoch)
    total = max(1, max(1, n_epochs) * per_epoch)
    local = max(0, int(global_step) - first_epoch * per_epoch)
    progress = min(1.0, local / float(total))
    cos01 = 0.5 * (1.0 + math.cos(math.pi * progress))
    return float(cfg.lr * float(min_mult + (lr_mult - min_mult) * cos01))


def sample_windows(corpus_u8: torch.Tensor, starts: torch.Tensor, seq_len: int) -> tuple:
    """(x, y) int64 of shape (len(starts), seq_len): x[i] = corpus[starts[i] : starts[i] + seq_len], y the same window one
    byte later -- one gather on the corpus's device, where the reference slices row by row on the host and copies
    every batch to the device.  starts[i] + seq_len must be below len(corpus)."""
    if corpus_u8.dim() != 1:
        raise ValueError("sample_windows: the corpus must be one-dimensional")
    idx = starts.to(device=corpus_u8.device, dtype=torch.long).unsqueeze(1) \
        + torch.arange(seq_len + 1, device=corpus_u8.device).unsqueeze(0)
    w = corpus_u8[idx].to(torch.long)
    return w[:, :-1].contiguous(), w[:, 1:].contiguous()


# ---- the end of an epoch: validation loss, parroting score, checkpoints ---------------------------------------------------

def load_corpus_as_u8(path: str, *, sanitize_ascii: bool, device=None) -> torch.Tensor:
    """The file's bytes as a 1-D uint8 tensor (reference :115-126); sanitize_ascii keeps \\n and printable ASCII and turns
    every other byte into a space.  `device` places the result (None: the CPU, as the reference)."""
    with open(path, "rb") as f:
        arr = np.frombuffer(f.read(), dtype=np.uint8)
    if sanitize_ascii:
        keep = (arr == 10) | ((arr >= 32) & (arr <= 126))
        arr = np.where(keep, arr, 32).astype(np.uint8)
    out = torch.from_numpy(arr.copy())
    return out if device is None else out.to(device)


@torch.no_grad()
def eval_loss(model, corpus_u8: torch.Tensor, starts: torch.Tensor, cfg, cutoff) -> float:
    """Mean cross-entropy over val_batches full batches of the fixed validation windows `starts` (reference :150-182): one
    torch.randperm(starts.numel()) draw from the global CPU generator picks the windows, so the same seed picks the
    reference's.  The windows are gathered on the corpus's device (sample_windows) and copied only when the model lives
    elsewhere; the per-batch losses (the native cross_entropy on a ROCm device) stay on the device and are averaged in
    float64 and read once at the end, where the reference reads one per batch.  Leaves the model in eval mode; 0.0 when
    `starts` holds no full batch."""
    model.eval()
    bs = int(cfg.batch_size)
    idx = torch.randperm(starts.numel())[: int(cfg.val_batches) * bs]
    sel = starts[idx.to(starts.device)]
    n_batches = sel.numel() // bs
    if n_batches == 0:
        return 0.0
    dev = next(model.parameters()).device
    losses = []
    for i in range(n_batches):
        x, y = sample_windows(corpus_u8, sel[i * bs:(i + 1) * bs], int(cfg.seq_len))
        if x.device != dev:
            x, y = x.to(dev, non_blocking=True), y.to(dev, non_blocking=True)
        losses.append(cross_entropy(model(x, cutoff=cutoff), y))        # F.cross_entropy on the CPU
    return float(torch.stack(losses).double().mean().item())


def parroting_picks(n_gen: int, cfg) -> np.ndarray:
    """The snippet starts the reference's parroting_score draws from a generation of n_gen bytes (:190-199): every
    parroting_stride-th start after the first 32 bytes, at most parroting_snips of them chosen without replacement by
    np.random.default_rng(123).  Empty when the generation is shorter than a snippet plus one byte."""
    L = int(cfg.parroting_snip_len)
    if n_gen < L + 1:
        return np.empty(0, np.int64)
    candidates = list(range(min(32, n_gen - L), n_gen - L, int(cfg.parroting_stride)))
    if not candidates:
        return np.empty(0, np.int64)
    rng = np.random.default_rng(123)
    return rng.choice(candidates, size=min(int(cfg.parroting_snips), len(candidates)), replace=False)


def parroting_score(corpus, gen_bytes: bytes, cfg) -> float:
    """Fraction of the picked parroting_snip_len-byte snippets of `gen_bytes` that occur verbatim in the corpus (reference
    :185-205; 0 = novel, 1 = copied).  `corpus`: bytes, a CPU uint8 tensor or a uint8 tensor on a ROCm device; the last
    is searched by ONE native pass for all snippets (find_snippets) where the reference scans the corpus once per
    snippet on the host.  The answers are read once."""
    picks = parroting_picks(len(gen_bytes), cfg)
    if picks.size == 0:
        return 0.0
    L = int(cfg.parroting_snip_len)
    gen = np.frombuffer(gen_bytes, dtype=np.uint8)
    snips = torch.from_numpy(gen[picks[:, None] + np.arange(L)[None, :]])
    if isinstance(corpus, torch.Tensor):
        snips = snips.to(corpus.device)
    hits = int((find_snippets(corpus, snips) >= 0).sum().item())
    return hits / float(len(picks))


def _sha256_file(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1024 * 1024), b""):
            h.update(chunk)
    return h.hexdigest()


def save_checkpoint(obj: Any, path: str) -> None:
    """torch.save and the file's SHA-256 in `path`.sha256 beside it (reference fft_lm/ckpt_io.py:40-45)."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save(obj, path)
    with open(path + ".sha256", "w", encoding="utf-8") as f:
        f.write(_sha256_file(path) + "\n")


def verify_checkpoint(path: str) -> bool:
    """True when `path` matches its .sha256 sidecar, False when there is none; a mismatch raises (ckpt_io.py:48-59)."""
    sha = path + ".sha256"
    if not os.path.exists(sha):
        return False
    with open(sha, "r", encoding="utf-8") as f:
        expected = f.read().strip().splitlines()[0]
    actual = _sha256_file(path)
    if expected != actual:
        raise RuntimeError(f"Checkpoint integrity check failed for {path}. "
                           f"Expected sha256={expected}, got sha256={actual}.")
    return True


def load_checkpoint(path: str, *, map_location="cpu") -> Any:
    """verify_checkpoint, then torch.load (pickle inside: only load files you wrote; ckpt_io.py:62-66)."""
    verify_checkpoint(path)
    return torch.load(path, map_location=map_location)


def checkpoint_state(model, opt, scaler, cfg, epoch: int) -> dict:
    """The dict the trainer saves (reference :883-893): epoch, model, opt, scaler (None without cfg.amp) and the config's
    fields.  `opt` and `scaler` may be None."""
    return {"epoch": epoch, "model": model.state_dict(), "opt": None if opt is None else opt.state_dict(),
            "scaler": scaler.state_dict() if scaler is not None and cfg.amp else None, "cfg": dict(cfg.__dict__)}


def config_from_checkpoint(ckpt: dict, cfg=None):
    """`cfg` (default: a fresh TrainConfig) with every field the checkpoint's saved config also has set from it; keys the
    config does not know are ignored (scripts/eval_ckpt.py:50-54)."""
    cfg = TrainConfig() if cfg is None else cfg
    if "cfg" in ckpt and isinstance(ckpt["cfg"], dict):
        for k, v in ckpt["cfg"].items():
            if hasattr(cfg, k):
                setattr(cfg, k, v)
    return cfg


def load_state_flexible(model, state: dict) -> tuple:
    """(resized, skipped): load a state dict whose tensors partly changed shape, e.g. after a seq_len change (reference
    :824-850).  Only 1-D `*gate_freq_logits` are resized (the common prefix is copied, the rest keeps the model's values);
    every other mismatch is skipped, unknown keys are ignored.  Both lists hold (key, saved shape, model shape)."""
    cur = model.state_dict()
    to_load, resized, skipped = {}, [], []
    for k, v in state.items():
        if k not in cur:
            continue
        if cur[k].shape == v.shape:
            to_load[k] = v
        elif k.endswith("gate_freq_logits") and v.ndim == 1 and cur[k].ndim == 1:
            tgt = cur[k].clone()
            n = min(tgt.numel(), v.numel())
            tgt[:n] = v[:n]
            to_load[k] = tgt
            resized.append((k, tuple(v.shape), tuple(tgt.shape)))
        else:
            skipped.append((k, tuple(v.shape), tuple(cur[k].shape)))
    model.load_state_dict(to_load, strict=False)
    return resized, skipped
