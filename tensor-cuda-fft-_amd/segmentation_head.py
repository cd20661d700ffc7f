"""Drop-in for `fft_lm.segmentation_head`: a 1-neuron head that predicts, for every byte, whether the word ends here
(the next byte is space, punctuation or a newline, or the sequence ends).

The labels come from one native launch on the tokens' device (functional.word_targets) instead of the reference's loop
over positions, and the head is the native 1-output row head (functional.narrow_head)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import functional as F_


class SegmentationHead(nn.Module):
    """hidden (B, T, d_model) -> boundary logits (B, T).  Zero-initialised."""

    def __init__(self, d_model: int):
        super().__init__()
        self.head = nn.Linear(d_model, 1)
        nn.init.zeros_(self.head.weight)
        nn.init.zeros_(self.head.bias)

    def forward(self, hidden: torch.Tensor) -> torch.Tensor:
        return F_.narrow_head(hidden, self.head.weight, self.head.bias).squeeze(-1)


def get_word_boundaries(text_bytes: torch.Tensor) -> torch.Tensor:
    """Word-boundary labels (B, T) fp32 of byte tokens (B, T), on the tokens' device: 1 where the next byte ends the
    word, and at the last position."""
    return F_.word_targets(text_bytes, phase=False, boundary=True)[1]


class SegmentedChunkLM(nn.Module):
    """`backbone` (with `cfg.d_model` and `forward_hidden(x, cutoff=...)`) plus a 256-way head over the last `chunk`
    positions and the segmentation head over all of them."""

    def __init__(self, backbone: nn.Module, chunk: int):
        super().__init__()
        self.backbone = backbone
        self.chunk = chunk
        d_model = backbone.cfg.d_model
        self.char_head = nn.Linear(d_model, 256)
        nn.init.normal_(self.char_head.weight, mean=0.0, std=0.02)
        nn.init.zeros_(self.char_head.bias)
        self.seg_head = SegmentationHead(d_model)

    def forward(self, x: torch.Tensor, cutoff: Optional[int] = None, return_seg_logits: Optional[bool] = None):
        """x (B, T) bytes -> char_logits (B, chunk, 256), and seg_logits (B, T) when `return_seg_logits` (None: in
        training mode)."""
        if return_seg_logits is None:
            return_seg_logits = self.training
        h = self.backbone.forward_hidden(x, cutoff=cutoff)
        char_logits = self.char_head(h[:, -self.chunk:, :])
        if return_seg_logits:
            return char_logits, self.seg_head(h)
        return char_logits


def compute_segmented_loss(char_logits: torch.Tensor, seg_logits: torch.Tensor, char_targets: torch.Tensor,
                           seg_targets: torch.Tensor, char_weight: float = 1.0, seg_weight: float = 0.1):
    """(total, char_loss, seg_loss): cross-entropy of the chunk plus `seg_weight` x the BCE of the boundary logits."""
    char_loss = nn.functional.cross_entropy(char_logits.reshape(-1, 256), char_targets.reshape(-1), reduction="mean")
    seg_loss = nn.functional.binary_cross_entropy_with_logits(seg_logits, seg_targets, reduction="mean")
    return char_weight * char_loss + seg_weight * seg_loss, char_loss, seg_loss
