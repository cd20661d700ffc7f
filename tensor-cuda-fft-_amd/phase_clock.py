"""Drop-in for `fft_lm.phase_clock`: words as half turns of a phase clock.  A 2-neuron head predicts, for every byte, the
point (cos, sin)(pi q / (n - 1)) of its position q in a word of n bytes, and (0, 0) on space and punctuation.

The targets come from one native launch on the tokens' device (functional.word_targets) instead of the reference's
per-byte `.item()` walk, and the head is the native 2-output row head (functional.narrow_head).

One deliberate difference: `generate_phase_targets` returns its result on the device of its input.  The reference always
returns a CPU tensor (its trainer then moves it with `.to(device)`, which is a no-op here)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import functional as F_


class PhaseClockHead(nn.Module):
    """hidden (B, T, d_model) -> phase vectors (B, T, 2): [..., 0] = cos, [..., 1] = sin.  Zero-initialised."""

    def __init__(self, d_model: int):
        super().__init__()
        self.head = nn.Linear(d_model, 2)
        nn.init.zeros_(self.head.weight)
        nn.init.zeros_(self.head.bias)

    def forward(self, hidden: torch.Tensor) -> torch.Tensor:
        return F_.narrow_head(hidden, self.head.weight, self.head.bias)


def generate_phase_targets(text_bytes: torch.Tensor) -> torch.Tensor:
    """Phase-clock targets (B, T, 2) fp32 of byte tokens (B, T), on the tokens' device."""
    return F_.word_targets(text_bytes, phase=True, boundary=False)[0]


class PhaseClockChunkLM(nn.Module):
    """`backbone` (with `cfg.d_model` and `forward_hidden(x, cutoff=...)`) plus a 256-way head over the last `chunk`
    positions and the phase-clock head over all of them."""

    def __init__(self, backbone: nn.Module, chunk: int):
        super().__init__()
        self.backbone = backbone
        self.chunk = chunk
        d_model = backbone.cfg.d_model
        self.char_head = nn.Linear(d_model, 256)
        nn.init.normal_(self.char_head.weight, mean=0.0, std=0.02)
        nn.init.zeros_(self.char_head.bias)
        self.phase_head = PhaseClockHead(d_model)

    def forward(self, x: torch.Tensor, cutoff: Optional[int] = None, return_phase_vectors: Optional[bool] = None):
        """x (B, T) bytes -> char_logits (B, chunk, 256), and phase_vectors (B, T, 2) when `return_phase_vectors`
        (None: in training mode)."""
        if return_phase_vectors is None:
            return_phase_vectors = self.training
        h = self.backbone.forward_hidden(x, cutoff=cutoff)
        char_logits = self.char_head(h[:, -self.chunk:, :])
        if return_phase_vectors:
            return char_logits, self.phase_head(h)
        return char_logits


def compute_phase_clock_loss(char_logits: torch.Tensor, phase_vectors: torch.Tensor, char_targets: torch.Tensor,
                             phase_targets: torch.Tensor, char_weight: float = 1.0, phase_weight: float = 5.0):
    """(total, char_loss, phase_loss): cross-entropy of the chunk plus `phase_weight` x the MSE of the phase vectors."""
    char_loss = nn.functional.cross_entropy(char_logits.reshape(-1, 256), char_targets.reshape(-1), reduction="mean")
    phase_loss = nn.functional.mse_loss(phase_vectors, phase_targets, reduction="mean")
    return char_weight * char_loss + phase_weight * phase_loss, char_loss, phase_loss
