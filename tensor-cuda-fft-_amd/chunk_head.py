"""Drop-in for `fft_lm.chunk_head`: ChunkLM, a backbone plus a head that predicts the next `chunk` bytes at once,
optionally conditioned on a SpectralEMA summary of the whole input window."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .spectral_ssm import EMAConfig, SpectralEMA


class ChunkLM(nn.Module):
    """`backbone` needs `embed.weight` (its second dimension is d_model) and `forward_hidden(x, cutoff=...)`."""

    def __init__(self, backbone: nn.Module, chunk: int, *, use_ema: bool = False, ema_chunk_len: int = 16,
                 ema_rho_init: float = 0.95, ema_mode: str = "aligned"):
        super().__init__()
        self.backbone = backbone
        self.chunk = int(chunk)
        d_model = backbone.embed.weight.shape[1]
        self.head = nn.Linear(d_model, 256 * self.chunk)
        self.use_ema = bool(use_ema)
        self.ema_chunk_len = int(ema_chunk_len)
        if self.use_ema:
            n_freqs = self.ema_chunk_len // 2 + 1
            self.ema = SpectralEMA(EMAConfig(n_freqs=n_freqs, rho_init=ema_rho_init, mode=ema_mode))
            self.ema_proj = nn.Linear(2 * n_freqs, d_model)
            nn.init.normal_(self.ema_proj.weight, mean=0.0, std=0.01)
            nn.init.zeros_(self.ema_proj.bias)
        nn.init.normal_(self.head.weight, mean=0.0, std=0.01)
        nn.init.zeros_(self.head.bias)

    def forward(self, x: torch.Tensor, cutoff: Optional[int] = None) -> torch.Tensor:
        """x (B, T) byte tokens -> logits (B, chunk, 256) of the next chunk."""
        last = self.backbone.forward_hidden(x, cutoff=cutoff)[:, -1, :]
        if self.use_ema and x.shape[1] // self.ema_chunk_len > 0:
            state = self.ema.scan_tokens(x, self.ema_chunk_len)                  # (B, F) complex: one launch on the GPU
            feat = torch.view_as_real(state).reshape(x.shape[0], -1)
            last = last + self.ema_proj(feat.to(last.dtype))
        return self.head(last).view(x.size(0), self.chunk, 256)


def vectorized_windows(corpus_u8: torch.Tensor, starts: torch.Tensor, seq_len: int, chunk: int):
    """x (B, seq_len) and its continuation y (B, chunk), both int64, gathered from a CPU byte corpus at `starts`."""
    offs = torch.arange(seq_len + chunk, dtype=torch.long)
    win = corpus_u8[starts.to(torch.long)[:, None] + offs[None, :]]
    return win[:, :seq_len].to(torch.long), win[:, seq_len:].to(torch.long)
