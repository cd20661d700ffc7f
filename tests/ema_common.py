"""Shared by the SpectralEMA tests and tests/golden/make_golden_ema.py: a restatement of the reference's op sequence
(fft_lm/spectral_ssm.py:71-125, fft_lm/chunk_head.py:48-69) in plain torch at ANY precision -- the reference itself pins
fp32 / complex64 inside its step, so its fp64 evaluation has to be restated -- plus the stub backbone and the byte
inputs of the chunk-head fixtures.  Nothing here imports the package under test or the reference."""
import math

import numpy as np
import torch
import torch.nn as nn

MIN_BIN = 0.25          # every bin of every byte chunk a test sees has |X| >= MIN_BIN (the reference is ill-conditioned below)


def step_ref(state, x, rho_logit, theta_raw, mode):
    """One step of the memory through abs / angle / exp, as the reference forms it (so autograd takes the same route,
    zero states and zero chunks included).  dtype follows `state`."""
    rdt = state.real.dtype
    rho = torch.sigmoid(rho_logit.to(rdt))
    keep = 1.0 - rho
    if mode == "polar":
        mag = rho[None] * state.abs() + keep[None] * x.abs()
        return mag.to(state.dtype) * torch.exp(1j * x.angle())
    if mode != "aligned":
        raise ValueError(mode)
    theta = math.pi * torch.tanh(theta_raw.to(rdt))
    a = (rho * torch.exp(1j * theta)).to(state.dtype)
    turn = torch.exp(1j * (x.angle() - state.angle())).to(state.dtype)
    return a[None] * (state * turn) + keep[None].to(state.dtype) * x


def scan_ref(chunks, rho_logit, theta_raw, mode, init=None):
    B, S, F = chunks.shape
    state = torch.zeros(B, F, dtype=chunks.dtype, device=chunks.device) if init is None else init
    for t in range(S):
        state = step_ref(state, chunks[:, t], rho_logit, theta_raw, mode)
    return state


def byte_chunks(x, L, rdt=torch.float64):
    """(B, T) byte tokens -> (B, T // L, L // 2 + 1) chunk spectra of x / 127.5 - 1."""
    B, T = x.shape
    S = T // L
    xx = x[:, :S * L].reshape(B, S, L).to(rdt) / 127.5 - 1.0
    return torch.fft.rfft(xx, dim=-1)


def conditioned_bytes(gen, B, T, L):
    """Uniform bytes (B, T) int64 with every full chunk redrawn until all its bins have |X| >= MIN_BIN (about a quarter
    of uniform chunks are redrawn); the trailing T % L bytes are plain uniform."""
    x = torch.randint(0, 256, (B, T), generator=gen, dtype=torch.int64)
    for b in range(B):
        for s in range(T // L):
            while byte_chunks(x[b:b + 1, s * L:(s + 1) * L], L).abs().min() < MIN_BIN:
                x[b, s * L:(s + 1) * L] = torch.randint(0, 256, (L,), generator=gen, dtype=torch.int64)
    assert T < L or float(byte_chunks(x, L).abs().min()) >= MIN_BIN
    return x


class StubBackbone(nn.Module):
    """The smallest thing ChunkLM accepts: an embedding (its width is d_model) and forward_hidden = one Linear."""

    def __init__(self, d_model=8):
        super().__init__()
        self.embed = nn.Embedding(256, d_model)
        self.mix = nn.Linear(d_model, d_model)

    def forward_hidden(self, x, cutoff=None):
        return self.mix(self.embed(x.long()))


def chunklm_ref(sd, x, L, chunk, mode, rdt=torch.float64, use_ema=True):
    """ChunkLM.forward over StubBackbone from a state_dict `sd` of tensors (cast to rdt here; leaves that require grad
    keep their graph)."""
    p = {k: v.to(rdt) for k, v in sd.items()}
    h = p["backbone.embed.weight"][x.long()] @ p["backbone.mix.weight"].T + p["backbone.mix.bias"]
    last = h[:, -1]
    if use_ema and x.shape[1] // L > 0:
        state = scan_ref(byte_chunks(x, L, rdt), p["ema.rho_logit"], p["ema.theta_raw"], mode)
        feat = torch.view_as_real(state).reshape(x.shape[0], -1)
        last = last + feat @ p["ema_proj.weight"].T + p["ema_proj.bias"]
    return (last @ p["head.weight"].T + p["head.bias"]).view(x.shape[0], chunk, 256)


def t(a, device=None, grad=False):
    out = torch.from_numpy(np.ascontiguousarray(a))
    if device is not None:
        out = out.to(device)
    return out.requires_grad_(True) if grad else out
