"""Drop-in for `fft_lm.spectral_ssm`: SpectralEMA, the frequency-domain state-space memory of the chunk head.

    aligned:  H' = rho e^{i theta} |H| u(X) + (1 - rho) X        rho = sigmoid(rho_logit), theta = pi tanh(theta_raw)
    polar:    H' = (rho |H| + (1 - rho) |X|) u(X)                u(X) = X / |X|, u = 1 at X == 0

The reference steps this in a Python loop of about fifteen small ops per chunk; on a ROCm device with complex64
chunks the whole scan is one launch of libsmx.so (functional.ema_scan), and `scan_tokens` forms the chunk spectra of
byte tokens inside that launch.  Everything the library does not take -- CPU tensors, complex128, `native = False`
-- runs the same step through torch's abs / angle / exp.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import functional as fn


@dataclass
class EMAConfig:
    n_freqs: int
    rho_init: float = 0.95
    theta_init: float = 0.0
    mode: str = "aligned"          # or "polar"


def _torch_step(state, x, rho, theta, mode: str):
    """One step in torch, by the same route as the reference (abs / angle / exp), so autograd agrees with it at zero
    states and zero chunks too."""
    cdt = torch.complex128 if rho.dtype == torch.float64 else torch.complex64
    if mode == "polar":
        mag = rho[None] * state.abs().to(rho.dtype) + (1.0 - rho)[None] * x.abs().to(rho.dtype)
        return mag.to(cdt) * torch.exp(1j * x.angle().to(rho.dtype)).to(cdt)
    a = (rho * torch.exp(1j * theta)).to(cdt)
    turn = torch.exp(1j * (x.angle().to(rho.dtype) - state.angle().to(rho.dtype))).to(cdt)
    return a[None] * (state * turn) + (1.0 - rho)[None].to(cdt) * x


class SpectralEMA(nn.Module):
    def __init__(self, cfg: EMAConfig):
        super().__init__()
        self.n_freqs = int(cfg.n_freqs)
        self.mode = str(cfg.mode)
        self.native = True             # False: every call takes the torch path
        rho0 = min(max(float(cfg.rho_init), 1e-4), 1 - 1e-4)
        self.rho_logit = nn.Parameter(torch.full((self.n_freqs,), math.log(rho0 / (1 - rho0)), dtype=torch.float32))
        self.theta_raw = nn.Parameter(torch.full((self.n_freqs,), float(cfg.theta_init), dtype=torch.float32))

    def _check_mode(self) -> None:
        fn._ema_mode(self.mode)        # ValueError for anything but 'aligned' / 'polar'

    def decay_params(self, device=None, dtype=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(a, rho, 1 - rho) with a = rho e^{i theta}."""
        rho = torch.sigmoid(self.rho_logit)
        theta = math.pi * torch.tanh(self.theta_raw)
        if device is not None or dtype is not None:
            rho, theta = rho.to(device=device, dtype=dtype), theta.to(device=device, dtype=dtype)
        return rho * torch.exp(1j * theta), rho, 1.0 - rho

    @torch.no_grad()
    def init_state(self, batch: int, device: torch.device, dtype: torch.dtype) -> torch.Tensor:
        return torch.zeros((batch, self.n_freqs), device=device, dtype=torch.complex64)

    def _takes(self, x: torch.Tensor, init: Optional[torch.Tensor] = None) -> bool:
        return (self.native and x.is_cuda and x.dtype == torch.complex64
                and self.rho_logit.is_cuda and self.rho_logit.dtype == torch.float32
                and (init is None or (init.is_cuda and init.dtype == torch.complex64)))

    def _torch_scan(self, chunks: torch.Tensor, init: Optional[torch.Tensor]) -> torch.Tensor:
        B, S, F = chunks.shape
        rdt = torch.float64 if chunks.dtype == torch.complex128 else torch.float32
        rho = torch.sigmoid(self.rho_logit).to(device=chunks.device, dtype=rdt)
        theta = (math.pi * torch.tanh(self.theta_raw)).to(device=chunks.device, dtype=rdt)
        state = torch.zeros((B, F), device=chunks.device, dtype=chunks.dtype) if init is None else init
        for t in range(S):
            state = _torch_step(state, chunks[:, t], rho, theta, self.mode)
        return state

    def update(self, state: torch.Tensor, fft_chunk: torch.Tensor) -> torch.Tensor:
        """One step from `state` (B, F) with `fft_chunk` (B, F): a scan of one chunk."""
        if state.shape != fft_chunk.shape:
            raise ValueError(f"state {tuple(state.shape)} and fft_chunk {tuple(fft_chunk.shape)} differ in shape")
        return self.scan(fft_chunk.unsqueeze(1), state)

    def scan(self, fft_chunks: torch.Tensor, init: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Final (B, F) state over fft_chunks (B, S, F) complex, from `init` (B, F) or zeros."""
        self._check_mode()
        B, S, F = fft_chunks.shape
        if F != self.n_freqs:
            raise ValueError(f"expected {self.n_freqs} bins, got {F}")
        if self._takes(fft_chunks, init):
            return fn.ema_scan(fft_chunks, self.rho_logit, self.theta_raw, self.mode, init)
        return self._torch_scan(fft_chunks, init)

    def scan_tokens(self, x: torch.Tensor, chunk_len: int) -> torch.Tensor:
        """scan() over the chunk spectra of byte tokens x (B, T): chunk t is rfft(x[:, t L : (t + 1) L] / 127.5 - 1)
        with L = chunk_len = 2 (n_freqs - 1) or that plus one; bytes past (T // L) L are ignored.  On a ROCm device
        (integer tokens, 2 <= L <= 64) the spectra are formed inside the scan launch and never stored."""
        self._check_mode()
        L = int(chunk_len)
        if L // 2 + 1 != self.n_freqs:
            raise ValueError(f"chunk_len {L} has {L // 2 + 1} bins, this memory has {self.n_freqs}")
        B, T = x.shape
        if (self.native and x.is_cuda and 2 <= L <= 64 and not x.is_floating_point() and not x.is_complex()
                and self.rho_logit.is_cuda and self.rho_logit.dtype == torch.float32):
            tok = x if x.dtype in (torch.uint8, torch.int64) else x.to(torch.int64)
            return fn.ema_scan_tokens(tok, L, self.rho_logit, self.theta_raw, self.mode)
        S = T // L
        xx = x[:, :S * L].reshape(B, S, L).to(torch.float32) / 127.5 - 1.0
        return self._torch_scan(torch.fft.rfft(xx, dim=-1), None)
