"""Drop-in mirrors of the sequence mixers of `fft_tensor.spectral_enhancements` that share the layer's
transform: `PhaseAwareSpectralMixing` (reference fft_tensor/spectral_enhancements.py:118-166)
and `MultiScaleSpectralFeatures` (:214-275).  Same constructors, attribute names and state_dict keys; the
rfft -> filter -> irfft of each runs as the fused HIP transform (functional.spectral_filter), not torch.fft.

The rest of the reference module is mirrored too, with the same constructors, buffers and state_dict keys:
`RotaryFrequencyEmbedding` (:20-71), `GatedSpectralUnit` (:74-116), `CausalFrequencyMask` (:169-211) and the block
that uses them all, `EnhancedSpectralBlock` (:278-333).  On a ROCm device with float32 tensors and an even D <= 1024
(functional.enh_supported) the row work of the block -- three LayerNorms, the pairwise rotation, the sigmoid gate blend
over gate_proj's 2D-wide LayerNorm, the dropouts and residual adds of lines 1-3 -- runs as three fused HIP row kernels
per direction (csrc/smx_enh.hip); the Linears stay on torch/hipBLASLt, phase_mixing / multi_scale on the native
transform.  Anything else (CPU, other dtypes, other D, `block.fuse_rows = False`) is the reference's own op sequence.

Documented deviation: in training mode the dropouts of lines 1-3 are drawn inside the row kernels from the library's
counter-based generator (keyed per call from torch's device generator, like SpectralMixingLayer): same distribution and
1/(1-p) scaling as nn.Dropout, different random bits, p quantised to 1/65536.  Line 4 keeps nn.Dropout.
`block.fuse_dropout = False` puts nn.Dropout back on every line (through the op-sequence path).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .functional import (DropoutState, enh_supported, gate_blend, hermitian_scale, phase_filter, residual_norm,
                         rope_norm, rope_rotate, spectral_filter)


def _native(x: torch.Tensor, *params) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and enh_supported(x.shape[-1])
            and all(p is None or (p.is_cuda and p.dtype == torch.float32) for p in params))


def _check_rope_shape(D: int, T: int, rotation: torch.Tensor) -> None:
    """The reference's failures, raised before any launch: an odd D cannot be paired (reshape(B, T, -1, 2), :61) and
    the table has max_seq_len rows and dim // 2 columns (:65)."""
    if D % 2:
        raise RuntimeError(f"RotaryFrequencyEmbedding pairs channels: D must be even, got {D}")
    if T > rotation.shape[0]:
        raise RuntimeError(f"sequence length {T} exceeds max_seq_len = {rotation.shape[0]}")
    if D // 2 > rotation.shape[1]:
        raise RuntimeError(f"D = {D} is wider than the rotation table ({2 * rotation.shape[1]} channels)")


class RotaryFrequencyEmbedding(nn.Module):
    """Channel pairs (x[2j], x[2j+1]) as complex numbers times e^{i t theta_j} (reference :20-71).  Buffers `inv_freq` and
    `rotation` ((max_seq_len, dim // 2) complex64) are built exactly as the reference builds them."""

    def __init__(self, dim, max_seq_len=4096, base=10000):
        super().__init__()
        self.dim = dim
        self.max_seq_len = max_seq_len
        inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim))            # :36
        self.register_buffer("inv_freq", inv_freq)
        t = torch.arange(max_seq_len).float()
        freqs = torch.outer(t, inv_freq)                                             # :41
        self.register_buffer("rotation", torch.polar(torch.ones_like(freqs), freqs))  # :44-45

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, D = x.shape
        _check_rope_shape(D, T, self.rotation)
        if _native(x) and self.rotation.dtype == torch.complex64 and self.rotation.is_cuda:
            return rope_rotate(x, self.rotation)
        x_pairs = x.reshape(B, T, -1, 2)                                             # :61-71
        x_complex = torch.complex(x_pairs[..., 0], x_pairs[..., 1])
        rotated = x_complex * self.rotation[:T, :x_complex.size(-1)].unsqueeze(0)
        return torch.stack([rotated.real, rotated.imag], dim=-1).reshape(B, T, D)


class GatedSpectralUnit(nn.Module):
    """gate, vt = LayerNorm(Linear(x)).chunk(2);  sigmoid(gate) value_proj(x) + (1 - sigmoid(gate)) vt  (reference
    :74-116; `num_gates` is kept and unused, as there).  On the native path the two Linears are torch GEMMs and the
    LayerNorm + gate + blend one row kernel each way."""

    def __init__(self, dim, num_gates=8):
        super().__init__()
        self.dim = dim
        self.num_gates = num_gates
        self.gate_proj = nn.Sequential(nn.Linear(dim, dim * 2), nn.LayerNorm(dim * 2))   # :88-91
        self.value_proj = nn.Linear(dim, dim)                                            # :94

    def _blend_native(self, x: torch.Tensor) -> bool:
        ln = self.gate_proj[1]
        return _native(x, ln.weight, ln.bias) and x.shape[-1] == self.dim

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._blend_native(x):
            ln = self.gate_proj[1]
            return gate_blend(self.gate_proj[0](x), self.value_proj(x), None, ln.weight, ln.bias, ln.eps)
        gate_input = self.gate_proj(x)                                                   # :105-114
        gate, value_transform = gate_input.chunk(2, dim=-1)
        gate = torch.sigmoid(gate)
        value = self.value_proj(x)
        return gate * value + (1 - gate) * value_transform


class CausalFrequencyMask(nn.Module):
    """x * causal_window[:T] with causal_window = 1 on the first max_seq_len // 2 positions (reference :169-211).
    A single multiply: it stays in torch."""

    def __init__(self, max_seq_len=4096):
        super().__init__()
        self.max_seq_len = max_seq_len
        self.register_buffer("causal_window", self._make_causal_window(max_seq_len))

    def _make_causal_window(self, seq_len):
        window = torch.zeros(seq_len)
        window[:seq_len // 2] = 1.0
        return window

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        T = x.size(1)
        return x * self.causal_window[:T].unsqueeze(0).unsqueeze(-1)


class PhaseAwareSpectralMixing(nn.Module):
    """irfft(polar(|X| * m, angle(X) + p)) with X = rfft(x, dim=1) and per-CHANNEL m, p (the reference
    indexes its (dim,) filters with `x_freq.size(-1)`, the channel count, :154-158).

    |X| m e^{i (angle X + p)} = X * (m e^{i p}): one complex constant per channel on every bin, so the
    whole layer is the fused transform with W[d, f] = m[d] e^{i p[d]} on all T//2 + 1 bins (irfft keeps
    only the real part of the DC / Nyquist products, exactly like the kernel).  The gradients of
    magnitude_filter / phase_filter follow from the native grad_W through this construction."""

    def __init__(self, dim, learnable=True):
        super().__init__()
        self.dim = dim
        if learnable:
            self.magnitude_filter = nn.Parameter(torch.ones(dim))       # reference :132-133
            self.phase_filter = nn.Parameter(torch.zeros(dim))
        else:
            self.register_buffer("magnitude_filter", torch.ones(dim))
            self.register_buffer("phase_filter", torch.zeros(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, D = x.shape
        K = T // 2 + 1
        m, p = self.magnitude_filter[:D], self.phase_filter[:D]         # :154, :157
        if x.is_cuda and m.dtype == torch.float32 and p.dtype == torch.float32:
            w_re, w_im = phase_filter(m, p, K, T)                        # one native launch (and one for its gradients)
        else:
            c = hermitian_scale(T, K, x.device)                          # irfft semantics (:164)
            w_re = (m * torch.cos(p)).unsqueeze(1) * c.unsqueeze(0)      # (D, K)
            w_im = (m * torch.sin(p)).unsqueeze(1) * c.unsqueeze(0)
        return spectral_filter(x, w_re, w_im, None, n_fft=T, k=K)


class MultiScaleSpectralFeatures(nn.Module):
    """Three band-limited copies of x -- rfft bins [0, K/4), [K/4, K/2), [K/2, K) -- each through its own
    Linear, then fused (reference :214-275).  The bands partition the spectrum, so with
    P_k = "keep the first k bins" (one fused native transform each):
        low = P_{K//4} x,   mid = P_{K//2} x - P_{K//4} x,   high = x - P_{K//2} x
    two pruned transforms instead of one full rfft and three full irffts."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.low_freq = nn.Linear(dim, dim)
        self.mid_freq = nn.Linear(dim, dim)
        self.high_freq = nn.Linear(dim, dim)
        self.fusion = nn.Linear(dim * 3, dim)
        self._w_cache = {}

    def _lowpass(self, x: torch.Tensor, k: int) -> torch.Tensor:
        if k <= 0:
            return torch.zeros_like(x)
        B, T, D = x.shape
        key = (T, D, k, x.device)
        w = self._w_cache.get(key)
        if w is None:
            w_re = hermitian_scale(T, k, x.device).unsqueeze(0).expand(D, k).contiguous()
            w = self._w_cache[key] = (w_re, torch.zeros_like(w_re))
        return spectral_filter(x, w[0], w[1], None, n_fft=T, k=k)

    def bands(self, x: torch.Tensor):
        """(low, mid, high) = the three irfft(...) of reference :246-262."""
        K = x.shape[1] // 2 + 1
        low_k, mid_k = K // 4, K // 2                                    # :242-243
        p_low = self._lowpass(x, low_k)
        p_mid = self._lowpass(x, mid_k)
        return p_low, p_mid - p_low, x - p_mid

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        low, mid, high = self.bands(x)
        combined = torch.cat([self.low_freq(low), self.mid_freq(mid), self.high_freq(high)], dim=-1)
        return self.fusion(combined)                                     # :265-272


class EnhancedSpectralBlock(nn.Module):
    """x1 = x + drop(rope(norm1(x))),  x2 = x1 + drop(phase_mixing(norm2(x1))),  x3 = x2 + drop(gated(norm3(x2))),
    x4 = x3 + drop(multi_scale(x3))  (reference :278-333, one shared `dropout`).

    Native path (fuse_rows = True, float32 on a ROCm device, even D <= 1024): lines 1-3 are three row kernels each way
    (functional.rope_norm, residual_norm, gate_blend) around the native phase_mixing transform and the two GEMMs of
    `gated`; line 4 is the torch expression above over the native multi_scale.  See the module docstring for the
    dropout deviation; fuse_dropout = False (in training with p > 0) and fuse_rows = False run the reference's op
    sequence."""

    def __init__(self, dim, dropout=0.1):
        super().__init__()
        self.rope = RotaryFrequencyEmbedding(dim)
        self.gated = GatedSpectralUnit(dim)
        self.phase_mixing = PhaseAwareSpectralMixing(dim)
        self.multi_scale = MultiScaleSpectralFeatures(dim)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.norm3 = nn.LayerNorm(dim)
        self.dropout = nn.Dropout(dropout)
        self.fuse_rows = True
        self.fuse_dropout = True
        self._drop_state = None

    def _fused_dropout_p(self) -> float:
        p = float(self.dropout.p)
        return p if (self.training and self.fuse_dropout and 0.0 < p < 1.0) else 0.0

    def _dropout_state(self, device: torch.device) -> DropoutState:
        if self._drop_state is None or self._drop_state.device != device:
            self._drop_state = DropoutState(device)
        return self._drop_state

    def _fusable(self, x: torch.Tensor) -> bool:
        active = self.training and self.dropout.p > 0.0
        norms = [t for n in (self.norm1, self.norm2, self.norm3, self.gated.gate_proj[1]) for t in (n.weight, n.bias)]
        return (self.fuse_rows and _native(x, *norms) and self.rope.rotation.dtype == torch.complex64
                and self.rope.rotation.is_cuda and x.shape[-1] == self.rope.dim and x.shape[-1] == self.gated.dim
                and not (active and self._fused_dropout_p() == 0.0))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, D = x.shape
        _check_rope_shape(D, T, self.rope.rotation)
        if not self._fusable(x):
            x = x + self.dropout(self.rope(self.norm1(x)))                                # :321
            x = x + self.dropout(self.phase_mixing(self.norm2(x)))                        # :324
            x = x + self.dropout(self.gated(self.norm3(x)))                               # :327
            return x + self.dropout(self.multi_scale(x))                                  # :330
        p = self._fused_dropout_p()
        ds = self._dropout_state(x.device) if p > 0.0 else None
        n1, n2, n3, g = self.norm1, self.norm2, self.norm3, self.gated
        x1, h2 = rope_norm(x, self.rope.rotation, n1.weight, n1.bias, n2.weight, n2.bias, n1.eps, n2.eps, p, ds)
        x2, h3 = residual_norm(x1, self.phase_mixing(h2), n3.weight, n3.bias, n3.eps, p, ds)
        ln = g.gate_proj[1]
        x3 = gate_blend(g.gate_proj[0](h3), g.value_proj(h3), x2, ln.weight, ln.bias, ln.eps, p, ds)
        return x3 + self.dropout(self.multi_scale(x3))                                   # :330
