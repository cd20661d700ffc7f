"""Drop-in mirror of the causal FFT convolution block the reference actually trains with:
`fft_lm.train_fixed_full.FixedSpectralBlock` (reference fft_lm/train_fixed_full.py:427-563) and the
frequency-domain multiply of its twin, `fft_lm.frequency_native.FrequencyConvFunc` (:80-121).
Same constructor, attribute names and state_dict keys (`kernel`, `gain`, `gate_freq_logits`, `ln.*`,
`gate_ctx.*`, `ffn_ln.*`, `ffn.*`), so reference checkpoints load unchanged.

The hot loop of that model is
    y = irfft( rfft(pad(x)) * k_freq * gain * sigmoid(gate_freq) * g_ctx * cutoff_mask, n )[:, :T]
Everything that multiplies the spectrum is either per frequency (shared by all channels) or per
(batch, channel), so the whole line is ONE fused native transform -- zero-padded load, full one-sided
spectrum incl. Nyquist, cropped store (functional.spectral_filter, smx_forward_ex) -- with
W[c, f] = H[f] * gain[c],  H = k_freq * sigmoid(gate_freq) * mask,  and the context gate applied to the
cropped output.  Parameter gradients follow from the native grad_W through that construction.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .functional import (_call, _stream, conv_response, conv_supported, hermitian_scale, rank_one_conv, sample_bytes,
                         spectral_filter)


def next_pow2(n: int) -> int:
    p = 1
    while p < n:
        p *= 2
    return p


_dft_cache: dict = {}


def _kernel_dft(n_fft: int, kernel_len: int, device) -> tuple:
    """(cos, -sin) matrices (n_fft//2+1, kernel_len), generated in fp64: the spectrum of the zero-padded
    causal kernel -- reference :511-513, rfft of n_fft points of which kernel_len are non-zero -- is a
    (1025 x 128) matrix-vector product at the default sizes, differentiable in the taps.  (The transform
    of the ACTIVATIONS is the native one; this is the filter's own 128-tap response.)"""
    key = (n_fft, kernel_len, str(device))
    m = _dft_cache.get(key)
    if m is None:
        f = torch.arange(n_fft // 2 + 1, dtype=torch.float64).unsqueeze(1)
        t = torch.arange(kernel_len, dtype=torch.float64).unsqueeze(0)
        ang = 2.0 * math.pi * ((f * t) % n_fft) / n_fft
        m = _dft_cache[key] = (torch.cos(ang).float().to(device), (-torch.sin(ang)).float().to(device))
    return m


def _kernel_response(kernel: torch.Tensor, n_fft: int) -> tuple:
    """(Re, Im) of rfft(zero-pad(kernel), n_fft) (reference :511-513), differentiable in the taps.  Short transforms:
    the cached DFT matrix product above.  From n_fft = 8192 on that matrix is 4 MiB and more per part and its two
    matrix-vector products cost more than the convolution's own launches (measured 2 x 352 us at n_fft = 65536):
    there the taps go through the native transform as a (1, K, 2) tensor, zero-padded load."""
    K = kernel.shape[0]
    if n_fft >= 8192 and kernel.is_cuda and kernel.dtype == torch.float32:
        from .functional import rfft
        spec = rfft(kernel.view(1, K, 1).expand(1, K, 2).contiguous(), n_fft)[0, :, 0]
        return spec.real, spec.imag
    cm, sm = _kernel_dft(n_fft, K, kernel.device)
    return cm @ kernel, sm @ kernel


def cutoff_mask(cutoff, fbins: int, transition_bins: int, device) -> "torch.Tensor | None":
    """Progressive frequency horizon of reference :540-551: 1 up to cutoff - trans, cosine roll-off, 0
    from cutoff on.  None when nothing is cut."""
    if cutoff is None:
        return None
    cutoff_idx = min(int(cutoff), fbins)
    if cutoff_idx >= fbins:
        return None
    trans = min(transition_bins, cutoff_idx)
    mask = torch.ones(fbins, device=device, dtype=torch.float32)
    start = cutoff_idx - trans
    if trans > 0:
        t = torch.linspace(0, 1, steps=trans, device=device, dtype=mask.dtype)
        mask[start:cutoff_idx] = 0.5 * (1.0 + torch.cos(torch.pi * t))
    mask[cutoff_idx:] = 0.0
    return mask


def causal_spectral_conv(x: torch.Tensor, kernel: torch.Tensor, gain: torch.Tensor,
                         gate_freq_logits: "torch.Tensor | None" = None,
                         g_ctx: "torch.Tensor | None" = None, cutoff=None,
                         transition_bins: int = 1) -> torch.Tensor:
    """Lines :507-555 of the reference block for x (B, T, C): causal linear convolution with the
    time-domain `kernel` via a zero-padded transform of length next_pow2(T + K - 1), per-channel `gain`,
    per-frequency sigmoid gate, per-(batch, channel) context gate `g_ctx` (already in [0, 1]) and the
    cosine cutoff mask; returns the first T samples.

    x may be fp32, bf16 or fp16.  For 2-byte x the parameters and g_ctx may each be fp32 or x's dtype; they are read
    as fp32 (`.float()`, so autograd returns each gradient in its own dtype) and the result is this function's on
    x.float(), rounded once to x's dtype: native 2-byte rows where rank_one_conv has them, the up-cast route
    x.float() -> fp32 op -> .to(dtype) on every other shape."""
    B, T, C = x.shape
    K = kernel.shape[0]
    n_fft = next_pow2(T + K - 1)                                           # :507-509
    fbins = n_fft // 2 + 1
    if x.dtype in (torch.bfloat16, torch.float16):
        kernel, gain = kernel.float(), gain.float()
        gate_freq_logits = None if gate_freq_logits is None else gate_freq_logits.float()
        g_ctx = None if g_ctx is None else g_ctx.float()
        if not (conv_supported(B, T, C, n_fft) and x.is_cuda):
            # shapes the convolution's own kernels do not take (odd C, n_fft < 512): spectral_filter is fp32-only
            return causal_spectral_conv(x.float(), kernel, gain, gate_freq_logits, g_ctx, cutoff,
                                        transition_bins).to(x.dtype)
    if conv_supported(B, T, C, n_fft) and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16, torch.float16):
        # n_fft 512 ... 65536: the convolution's own kernels -- the packed
        # spectrum times the Hermitian extension of H, gain x context gate at the store (smx_conv_*).
        # H = k_freq (:511-513) x sigmoid(gate) (:529) x mask (:551): one native launch (and one for its gradients)
        mask = cutoff_mask(cutoff, fbins, transition_bins, x.device)
        if kernel.dtype == torch.float32 and (gate_freq_logits is None or gate_freq_logits.dtype == torch.float32):
            h_re, h_im = conv_response(kernel, gate_freq_logits, mask, n_fft)
        else:
            h_re, h_im = _kernel_response(kernel, n_fft)
            per_f = None
            if gate_freq_logits is not None:
                per_f = torch.sigmoid(gate_freq_logits[:fbins])
            if mask is not None:
                per_f = mask if per_f is None else per_f * mask
            if per_f is not None:
                h_re, h_im = h_re * per_f, h_im * per_f
        s = gain.unsqueeze(0).expand(B, C) if g_ctx is None else gain.unsqueeze(0) * g_ctx   # :522, :533-536
        return rank_one_conv(x, h_re, h_im, s.contiguous(), n_fft)        # (2-byte x: y in x's dtype)
    h_re, h_im = _kernel_response(kernel, n_fft)                           # k_freq, :511-513
    scale = hermitian_scale(n_fft, fbins, x.device)                        # irfft semantics, :553
    if gate_freq_logits is not None:
        scale = scale * torch.sigmoid(gate_freq_logits[:fbins])            # :529
    mask = cutoff_mask(cutoff, fbins, transition_bins, x.device)
    if mask is not None:
        scale = scale * mask                                               # :551
    h_re, h_im = h_re * scale, h_im * scale
    w_re = gain.unsqueeze(1) * h_re.unsqueeze(0)                           # (C, fbins), :522
    w_im = gain.unsqueeze(1) * h_im.unsqueeze(0)
    # :515-519, :553-555; the context gate (:533-536) rides along as the per-(batch, channel) factor
    return spectral_filter(x, w_re, w_im, None, n_fft=n_fft, k=fbins, row_scale=g_ctx)


def _causal_conv_torch(x, kernel, gain, gate_freq_logits, g_ctx, cutoff, transition_bins):
    """causal_spectral_conv's line through torch.fft, for CPU tensors only (as spectral_ssm.py's torch path: the
    library has no CPU kernels, and on a ROCm device the native line is the only one)."""
    B, T, C = x.shape
    K = kernel.shape[0]
    n_fft = next_pow2(T + K - 1)
    fbins = n_fft // 2 + 1
    h = torch.fft.rfft(kernel.to(x.dtype), n=n_fft) * torch.sigmoid(gate_freq_logits[:fbins]).to(x.dtype)
    mask = cutoff_mask(cutoff, fbins, transition_bins, x.device)
    if mask is not None:
        h = h * mask.to(x.dtype)
    y = torch.fft.irfft(torch.fft.rfft(x, n=n_fft, dim=1) * h.view(1, -1, 1), n=n_fft, dim=1)[:, :T]
    return y * (gain.unsqueeze(0) * g_ctx).unsqueeze(1)


class FixedSpectralBlock(nn.Module):
    """Pre-norm causal spectral mixing + gated valve + FFN residual (reference :427-563).  A CPU input takes the same
    line through torch.fft (streaming.py's torch path and the CPU tests run on it)."""

    def __init__(self, d_model: int, seq_len: int, kernel_len: int, transition_bins: int, dropout: float = 0.1):
        super().__init__()
        self.ln = nn.LayerNorm(d_model)
        self.drop = nn.Dropout(dropout)
        self.seq_len = seq_len
        self.kernel_len = kernel_len
        self.transition_bins = int(max(1, transition_bins))
        self.kernel = nn.Parameter(torch.zeros(kernel_len))
        nn.init.normal_(self.kernel, mean=0.0, std=0.001)                  # :447-448
        self.gain = nn.Parameter(torch.ones(d_model))                      # :451
        self.max_freq_bins = next_pow2(int(seq_len + kernel_len - 1)) // 2 + 1      # :468-472
        self.gate_freq_logits = nn.Parameter(torch.ones(self.max_freq_bins) * 2.0)  # :475
        self.gate_ctx = nn.Linear(d_model, d_model)
        nn.init.zeros_(self.gate_ctx.weight)
        nn.init.constant_(self.gate_ctx.bias, 2.0)                         # :478-480
        hidden = d_model * 2
        self.ffn_ln = nn.LayerNorm(d_model)
        self.ffn = nn.Sequential(nn.Linear(d_model, hidden), nn.GELU(), nn.Dropout(dropout),
                                 nn.Linear(hidden, d_model))
        for m in self.ffn:
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0.0, std=0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x: torch.Tensor, cutoff: "int | None" = None) -> torch.Tensor:
        residual = x
        x = self.ln(x)
        g_ctx = torch.sigmoid(self.gate_ctx(x.mean(dim=1)))                # :532-533
        if x.is_cuda:
            y = causal_spectral_conv(x, self.kernel, self.gain, self.gate_freq_logits, g_ctx, cutoff,
                                     self.transition_bins)
        else:
            y = _causal_conv_torch(x, self.kernel, self.gain, self.gate_freq_logits, g_ctx, cutoff,
                                   self.transition_bins)
        x = residual + self.drop(y)                                        # :557-558
        return x + self.drop(self.ffn(self.ffn_ln(x)))                     # :561-562


class FrequencyConvFunc(torch.autograd.Function):
    """y_freq = x_freq * kernel_freq[None, :, None] * gain[None, None, :] with the reference's hand-written
    backward (fft_lm/frequency_native.py:80-121), on the native complex-multiply kernels
    (smx_cmul / smx_cmul_grad_w).  x_freq (B, F, C) complex64, kernel_freq (F) complex64, gain (C) fp32."""

    @staticmethod
    def forward(ctx, x_freq, kernel_freq, gain):
        if not x_freq.is_cuda or x_freq.dtype != torch.complex64:
            raise TypeError("x_freq must be a complex64 tensor on a ROCm device")
        x = x_freq.resolve_conj().contiguous()
        w = (kernel_freq.to(torch.complex64).unsqueeze(1) * gain.unsqueeze(0)).contiguous()    # (F, C)
        out = torch.empty_like(x)
        _call(x.device, "smx_cmul", x.data_ptr(), w.data_ptr(), out.data_ptr(), x.shape[0], w.numel(), 0,
              _stream(x.device))
        ctx.save_for_backward(x, kernel_freq, gain, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, kernel_freq, gain, w = ctx.saved_tensors
        g = grad_output.resolve_conj().contiguous()
        B, inner = x.shape[0], w.numel()
        grad_x = torch.empty_like(x)
        s_conj = torch.empty_like(w)          # sum_b g * conj(x)
        s_plain = torch.empty_like(w)         # sum_b g * x
        xc = x.conj().resolve_conj()
        s = _stream(x.device)
        _call(x.device, "smx_cmul", g.data_ptr(), w.data_ptr(), grad_x.data_ptr(), B, inner, 1, s)     # :111
        _call(x.device, "smx_cmul_grad_w", x.data_ptr(), g.data_ptr(), s_conj.data_ptr(), B, inner, s)
        _call(x.device, "smx_cmul_grad_w", xc.data_ptr(), g.data_ptr(), s_plain.data_ptr(), B, inner, s)
        grad_kernel = (s_conj * gain.unsqueeze(0)).sum(dim=1)                                 # :114
        grad_gain = (s_plain * kernel_freq.unsqueeze(1)).real.sum(dim=0)                      # :117
        return grad_x, grad_kernel, grad_gain


@dataclass
class LMConfig:
    """The fields of the reference's TrainConfig that FixedSpectralLM reads, with its defaults (reference :38-49, :63)."""
    vocab_size: int = 256
    d_model: int = 512
    n_layers: int = 6
    seq_len: int = 1024
    kernel_len: int = 128
    jpeg_transition: int = 32
    bicameral: bool = False
    frequency_native: bool = False


class FixedSpectralLM(nn.Module):
    """Byte embedding, n_layers spectral blocks, final LayerNorm, logits through the embedding matrix (weight tying):
    reference :566-618, the backbone ChunkLM wraps.  `cfg` is an LMConfig, the reference's TrainConfig or any object
    with LMConfig's fields; state_dict keys `embed.*`, `blocks.{i}.*`, `ln_f.*` as in the reference."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.embed = nn.Embedding(cfg.vocab_size, cfg.d_model)
        if cfg.bicameral:                                                  # :573-583
            from .frequency_native import BicameralBlock as block_class
        elif cfg.frequency_native:
            from .frequency_native import FrequencyNativeBlock as block_class
        else:
            block_class = FixedSpectralBlock
        self.blocks = nn.ModuleList([
            block_class(cfg.d_model, seq_len=cfg.seq_len, kernel_len=cfg.kernel_len,
                        transition_bins=cfg.jpeg_transition, dropout=0.1)
            for _ in range(cfg.n_layers)])
        self.ln_f = nn.LayerNorm(cfg.d_model)

    def forward(self, x: torch.Tensor, cutoff: "int | None" = None) -> torch.Tensor:
        """x (B, T) long -> logits (B, T, vocab_size)."""
        return torch.matmul(self.forward_hidden(x, cutoff=cutoff), self.embed.weight.t())

    def forward_hidden(self, x: torch.Tensor, cutoff: "int | None" = None) -> torch.Tensor:
        """x (B, T) long -> final hidden states (B, T, d_model)."""
        h = self.embed(x)
        for blk in self.blocks:
            h = blk(h, cutoff=cutoff)
        return self.ln_f(h)


@dataclass
class SampleConfig:
    """The generation fields of the reference's TrainConfig with its defaults (reference :65-78), and the seq_len
    `generate` reads beside them."""
    seq_len: int = 1024
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


@torch.no_grad()
def generate(model: "FixedSpectralLM", prompt: str, cfg, *, cutoff: "int | None" = None, generator=None) -> str:
    """The reference's byte-by-byte `generate` (reference :621-704) on the model's device: per emitted byte ONE model
    forward over the last cfg.seq_len bytes of a device-resident context and ONE sampler call
    (functional.sample_bytes: a single launch on a ROCm device) -- no logit and no id is read by the host inside the
    loop, where the reference synchronises several times per byte; the text is decoded once at the end.  `cfg`: a
    SampleConfig, the reference's TrainConfig or any object with SampleConfig's fields.  The uniforms come from
    torch.rand on the device (`generator`, or the device's default one), one per byte.
    Two limits the reference does not have: 1 <= repetition_window <= 65536 (a window of 0 there means the whole
    text), and max_run_length <= repetition_window (the run is looked for inside the window)."""
    model.eval()
    ctx = list(prompt.encode("utf-8", errors="ignore")) or [32]
    T, window, max_new = int(cfg.seq_len), int(cfg.repetition_window), int(cfg.max_new)
    max_run = int(cfg.max_run_length or 0)
    if not 1 <= window <= 65536:
        raise ValueError(f"generate: repetition_window must be in 1..65536, got {window}")
    if max_run > window:
        raise ValueError(f"generate: max_run_length = {max_run} is longer than repetition_window = {window}")
    dev = model.embed.weight.device
    n0 = len(ctx)
    buf = torch.empty(n0 + max(max_new, 0), dtype=torch.long, device=dev)
    buf[:n0] = torch.tensor(ctx, dtype=torch.long, device=dev)
    top_p = 1.0 if cfg.top_p is None else float(cfg.top_p)
    for n in range(n0, n0 + max_new):
        logits = model(buf[max(0, n - T):n].unsqueeze(0), cutoff=cutoff)[:, -1]
        u = torch.rand(1, dtype=torch.float32, device=dev, generator=generator)
        buf[n:n + 1] = sample_bytes(logits, buf[max(0, n - window):n], u, temperature=cfg.temperature, top_p=top_p,
                                    top_k=int(cfg.top_k or 0), repetition_penalty=cfg.repetition_penalty,
                                    presence_penalty=cfg.presence_penalty or 0.0,
                                    frequency_penalty=cfg.frequency_penalty or 0.0, ascii_only=bool(cfg.ascii_only),
                                    ban_cr=bool(cfg.ban_cr), max_run_length=max_run)
    return bytes(buf.tolist()).decode("utf-8", errors="replace")
