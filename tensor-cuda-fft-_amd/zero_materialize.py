"""Mirror of `fft_tensor.zero_materialize` (reference fft_tensor/zero_materialize.py): ConvolutionTheoremMatMul
(frequency_linear :44-86, frequency_conv1d :89-150, frequency_conv2d :153-205, frequency_conv3d :208-261,
frequency_linear_batched :264-317), WirtingerAutograd (:320-372), FrequencyLinearLayer (:375-452), LogarithmicQuantizer
(:455-568) and the functions frequency_linear / frequency_conv1d (:572-590).  Names, arguments, defaults and state_dict keys
are the reference's.

What the reference computes is kept; how is not.  It multiplies a broadcast (B, N, D_in, D_out) or (B, C_out, C_in, L...)
complex product and reduces it; nothing of that size is formed here:

* frequency_linear.  Re(ifft(fft(x, -1) @ W, -1)) = x @ M with M = ifft(fft(W, dim=0), dim=1) (the transforms are linear
  and act on different axes than the sum), and for real x only Re(M) matters: one real GEMM and a D_in x D_out transform
  of the weight.  On a ROCm device M comes from the package's differentiable sequence transform (functional.seq_fft on
  the (1, D_in, D_out) view for axis 0, its conjugate form on the transposed weight for axis 1), so no FFT library runs
  and the op is differentiable in w_freq; the GEMM stays on torch.
* the convolutions.  x goes to channels-innermost layout once, each spatial axis is transformed as the middle axis of a
  view (functional.seq_fft), the bins are contracted against w_freq permuted to (bins, C_in, C_out) by
  functional.bin_contract, and the way back is the conjugate form of the same transforms.  Differentiable in x and w_freq.
* CPU tensors (and other dtypes) run torch.fft with a matmul / einsum, again without the broadcast product.

The reference's behaviour is mirrored as it is, quirks included; each docstring says which."""
import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import functional as _fn


def _native(x: torch.Tensor, w_freq: torch.Tensor) -> bool:
    return (x.is_cuda and w_freq.device == x.device and x.dtype in (torch.float32, torch.complex64)
            and w_freq.dtype == torch.complex64 and x.numel() > 0 and w_freq.numel() > 0)


def _weight_matrix(w_freq: torch.Tensor) -> torch.Tensor:
    """conj(M)^T * D_out for M = ifft(fft(w_freq, dim=0), dim=1), as (D_out, D_in) complex64, on the native transform:
    ifft(A, dim) = conj(fft(conj(A), dim)) / n, and the caller folds the conjugate and 1 / n in."""
    D_in, D_out = w_freq.shape
    f0 = _fn.seq_fft(w_freq.reshape(1, D_in, D_out)) if D_in > 1 else w_freq.reshape(1, D_in, D_out)
    a = f0.transpose(1, 2).conj()                                        # (1, D_out, D_in)
    return (_fn.seq_fft(a) if D_out > 1 else a.resolve_conj()).squeeze(0)


def _walk_axes(z: torch.Tensor, spatial: Tuple[int, ...]) -> torch.Tensor:
    """fftn over the spatial axes of a contiguous (B, *spatial, C) complex64 tensor: axis i is the middle axis of the view
    (B prod(spatial[:i]), spatial[i], prod(spatial[i+1:]) C); nothing is transposed.  Axes of length 1 are skipped."""
    shape = z.shape
    B, C = shape[0], shape[-1]
    for i, n in enumerate(spatial):
        if n > 1:
            z = _fn.seq_fft(z.reshape(B * math.prod(spatial[:i]), n, math.prod(spatial[i + 1:]) * C))
    return z.reshape(shape)


def _spectral_conv(x: torch.Tensor, w_freq: torch.Tensor) -> torch.Tensor:
    """Re(ifftn(sum_c fftn(x)[b, c] w_freq[o, c])) over the spatial axes: x (B, C_in, *S), w_freq (C_out, C_in, *S),
    the result (B, C_out, *S)."""
    S = tuple(x.shape[2:])
    nd = len(S)
    if not _native(x, w_freq) or tuple(w_freq.shape[2:]) != S:
        dims = tuple(range(-nd, 0))
        letters = "xyz"[:nd]
        y_freq = torch.einsum(f"bi{letters},oi{letters}->bo{letters}", torch.fft.fftn(x, dim=dims), w_freq)
        return torch.fft.ifftn(y_freq, dim=dims).real
    B, C_in = x.shape[:2]
    C_out = w_freq.shape[0]
    P = math.prod(S)
    sp = tuple(range(2, 2 + nd))
    xs = _walk_axes(x.permute(0, *sp, 1).to(torch.complex64).contiguous(), S)                # (B, *S, C_in)
    ws = w_freq.permute(*sp, 1, 0).reshape(P, C_in, C_out)
    ys = _fn.bin_contract(xs.reshape(B, P, C_in), ws).reshape(B, *S, C_out)
    y = _walk_axes(ys.conj().resolve_conj(), S).real / P                                     # Re(conj(fftn(conj Y))) / P
    return y.permute(0, nd + 1, *range(1, nd + 1))


class ConvolutionTheoremMatMul:
    @staticmethod
    def frequency_linear(x: torch.Tensor, w_freq: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x (B, N, D_in), w_freq (D_in, D_out) complex, bias (D_out): Re(ifft(fft(x, dim=-1) @ w_freq, dim=-1)) + bias,
        (B, N, D_out).  Note what this is: w_freq is applied to the spectrum of x along the FEATURE axis, which equals
        x @ ifft(fft(w_freq, dim=0), dim=1); it is not x @ ifft(w_freq).  Computed as that one product (see the module's
        docstring); the reference's (B, N, D_in, D_out) product is never formed.  Differentiable in x, w_freq and bias."""
        B, N, D_in = x.shape
        D_in2, D_out = w_freq.shape
        assert D_in == D_in2
        if _native(x, w_freq):
            m = _weight_matrix(w_freq)                                   # (D_out, D_in): conj(M)^T D_out
            if x.is_complex():
                y = torch.matmul(x, m.conj().transpose(0, 1)).real / D_out
            else:
                y = F.linear(x, m.real) / D_out
        else:
            y = torch.fft.ifft(torch.matmul(torch.fft.fft(x, dim=-1), w_freq), dim=-1).real
        if bias is not None:
            y = y + bias
        return y

    @staticmethod
    def frequency_conv1d(x: torch.Tensor, w_freq: torch.Tensor, stride: int = 1, padding: int = 0) -> torch.Tensor:
        """x (B, C_in, L), w_freq (C_out, C_in, K) complex -- a SPECTRUM: with L' = L + 2 padding it is zero-padded (or
        cut) along its last axis to L' bins IN THE FREQUENCY DOMAIN, as the reference does, so it is the spectrum of a
        kernel only when K == L'.  y = Re(ifft(sum_c fft(x_pad)[b, c] w_freq[o, c])), L' samples; with padding > 0 the
        samples [K // 2, L' - (K - K // 2 - 1)) are kept, K being the ORIGINAL last size of w_freq (an empty result when
        that range is empty); then every stride-th sample."""
        B, C_in, L = x.shape
        C_out, C_in2, K = w_freq.shape
        assert C_in == C_in2
        if padding > 0:
            x = F.pad(x, (padding, padding))
            L = L + 2 * padding
        if w_freq.shape[-1] < L:
            w_freq = F.pad(w_freq, (0, L - w_freq.shape[-1]))
        elif w_freq.shape[-1] > L:
            w_freq = w_freq[:, :, :L]
        y = _spectral_conv(x, w_freq)
        if padding > 0:
            crop_start = K // 2
            crop_end = y.shape[-1] - (K - K // 2 - 1)
            y = y[:, :, crop_start:crop_end]
        if stride > 1:
            y = y[:, :, ::stride]
        return y

    @staticmethod
    def frequency_conv2d(x: torch.Tensor, w_freq: torch.Tensor, stride: Tuple[int, int] = (1, 1),
                         padding: Tuple[int, int] = (0, 0)) -> torch.Tensor:
        """x (B, C_in, H, W), w_freq (C_out, C_in, Kh, Kw) complex, a spectrum zero-padded in the frequency domain to the
        padded input's (H', W') (a larger one fails, as in the reference): Re(ifft2(sum_c fft2(x_pad) w_freq)), all
        (H', W') samples (no crop, as in the reference), then the strides."""
        B, C_in, H, W = x.shape
        C_out, C_in2, Kh, Kw = w_freq.shape
        assert C_in == C_in2
        if padding[0] > 0 or padding[1] > 0:
            x = F.pad(x, (padding[1], padding[1], padding[0], padding[0]))
            H = H + 2 * padding[0]
            W = W + 2 * padding[1]
        if w_freq.shape[-2] < H or w_freq.shape[-1] < W:
            pad_h = max(0, H - w_freq.shape[-2])
            pad_w = max(0, W - w_freq.shape[-1])
            w_freq = F.pad(w_freq, (0, pad_w, 0, pad_h))
        y = _spectral_conv(x, w_freq)
        if stride[0] > 1 or stride[1] > 1:
            y = y[:, :, ::stride[0], ::stride[1]]
        return y

    @staticmethod
    def frequency_conv3d(x: torch.Tensor, w_freq: torch.Tensor, stride: Tuple[int, int, int] = (1, 1, 1),
                         padding: Tuple[int, int, int] = (0, 0, 0)) -> torch.Tensor:
        """x (B, C_in, D, H, W), w_freq (C_out, C_in, Kd, Kh, Kw) complex: frequency_conv2d with one more axis."""
        B, C_in, D, H, W = x.shape
        C_out, C_in2, Kd, Kh, Kw = w_freq.shape
        assert C_in == C_in2
        if padding[0] > 0 or padding[1] > 0 or padding[2] > 0:
            x = F.pad(x, (padding[2], padding[2], padding[1], padding[1], padding[0], padding[0]))
            D = D + 2 * padding[0]
            H = H + 2 * padding[1]
            W = W + 2 * padding[2]
        if w_freq.shape[-3] < D or w_freq.shape[-2] < H or w_freq.shape[-1] < W:
            pad_d = max(0, D - w_freq.shape[-3])
            pad_h = max(0, H - w_freq.shape[-2])
            pad_w = max(0, W - w_freq.shape[-1])
            w_freq = F.pad(w_freq, (0, pad_w, 0, pad_h, 0, pad_d))
        y = _spectral_conv(x, w_freq)
        if stride[0] > 1 or stride[1] > 1 or stride[2] > 1:
            y = y[:, :, ::stride[0], ::stride[1], ::stride[2]]
        return y

    @staticmethod
    def frequency_linear_batched(x_batch: torch.Tensor, w_freq: torch.Tensor, bias: Optional[torch.Tensor] = None,
                                 chunk_size: int = 32) -> torch.Tensor:
        """frequency_linear's values.  The reference walks the batch in chunks to bound its broadcast product; there is
        none here, so `chunk_size` is accepted and not used.  As in the reference the result has x_batch's dtype (the
        real part, for a complex input, is cast back to it)."""
        y = ConvolutionTheoremMatMul.frequency_linear(x_batch, w_freq, None).to(x_batch.dtype)
        if bias is not None:
            y = y + bias
        return y


class WirtingerAutograd(torch.autograd.Function):
    """The reference's elementwise complex product with its hand-written backward: forward x_freq * w_freq; backward
    grad_x = grad_output conj(w_freq), grad_w = grad_output conj(x_freq) -- without a reduction over broadcast axes, as in
    the reference, so the operands must have one shape for autograd to accept the gradients."""

    @staticmethod
    def forward(ctx, x_freq: torch.Tensor, w_freq: torch.Tensor) -> torch.Tensor:
        ctx.save_for_backward(x_freq, w_freq)
        return x_freq * w_freq

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        x_freq, w_freq = ctx.saved_tensors
        return grad_output * torch.conj(w_freq), grad_output * torch.conj(x_freq)


class FrequencyLinearLayer(torch.nn.Module):
    """The reference's FrequencyLinearLayer: weight_freq, an (out_features, in_features) complex spectrum with all but the
    k = int(in_features * sparsity) largest bins of each row zeroed at construction, applied by frequency_linear.  State:
    `weight_freq`, `bias` (learn_phase=True) or `weight_magnitude`, `bias` and the buffer `weight_phase`; a reference
    state_dict loads with strict=True.  The initial draw is made on the CPU exactly as the reference makes it, so a seed
    gives the same layer; the reference's per-row loop that copies the kept bins is one scatter.
    Mirrored as they are:
    * forward hands the (out, in) weight to frequency_linear as its (D_in, D_out) operand, so only a SQUARE layer runs
      (AssertionError otherwise);
    * k = int(in_features * sparsity) is 0 below 100 features at the default sparsity 0.01: a zero weight;
    * compress_ratio reads weight_freq, so it needs learn_phase=True (AttributeError otherwise) and a non-zero weight."""

    def __init__(self, in_features: int, out_features: int, sparsity: float = 0.01, bias: bool = True,
                 learn_phase: bool = True):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.sparsity = sparsity
        self.learn_phase = learn_phase
        spatial_init = torch.randn(out_features, in_features) * 0.02
        freq_init = torch.fft.fft(spatial_init, dim=-1)
        k = int(in_features * sparsity)
        _, topk_indices = torch.topk(torch.abs(freq_init), k, dim=-1)
        sparse_freq = torch.zeros_like(freq_init).scatter_(1, topk_indices, freq_init.gather(1, topk_indices))
        if learn_phase:
            self.weight_freq = torch.nn.Parameter(sparse_freq)
        else:
            self.weight_magnitude = torch.nn.Parameter(torch.abs(sparse_freq))
            self.register_buffer('weight_phase', torch.angle(sparse_freq))
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(out_features))
        else:
            self.register_parameter('bias', None)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.learn_phase:
            w_freq = self.weight_freq
        else:
            w_freq = self.weight_magnitude * torch.exp(1j * self.weight_phase)
        return ConvolutionTheoremMatMul.frequency_linear(x, w_freq, self.bias)

    def compress_ratio(self) -> float:
        total = self.in_features * self.out_features
        sparse = torch.count_nonzero(torch.abs(self.weight_freq) > 1e-8).item()
        return total / sparse


class LogarithmicQuantizer:
    """The reference's 8-bit logarithmic codec, sign(1) + log-mantissa(7), on functional.log8_encode / log8_decode and
    their one-pass complex forms (csrc/smx_quant.hip on a ROCm device, the reference's op sequence elsewhere)."""

    @staticmethod
    def log8_encode(x: torch.Tensor) -> torch.Tensor:
        return _fn.log8_encode(x)

    @staticmethod
    def log8_decode(encoded: torch.Tensor) -> torch.Tensor:
        return _fn.log8_decode(encoded)

    @staticmethod
    def compress_sparse_freq(freq_coeffs: torch.Tensor, indices: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(compressed_real, compressed_imag) of the complex coefficients; `indices` is accepted and not used, as in
        the reference."""
        return _fn.log8_encode_complex(freq_coeffs)

    @staticmethod
    def decompress_sparse_freq(compressed_real: torch.Tensor, compressed_imag: torch.Tensor, indices: torch.Tensor,
                               shape: Tuple[int, ...]) -> torch.Tensor:
        """A complex64 tensor of `shape`, zero except at `indices` (indexing along the first axis, as `t[indices] = v`
        does), where it holds the decoded coefficients.  The one stated deviation: the result is created on the inputs'
        device; the reference creates it on the CPU, which fails for device inputs."""
        coeffs = _fn.log8_decode_complex(compressed_real, compressed_imag)
        freq_coeffs = torch.zeros(shape, dtype=torch.complex64, device=coeffs.device)
        freq_coeffs[indices] = coeffs
        return freq_coeffs


def frequency_linear(x: torch.Tensor, w_freq: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ConvolutionTheoremMatMul.frequency_linear"""
    return ConvolutionTheoremMatMul.frequency_linear(x, w_freq, bias)


def frequency_conv1d(x: torch.Tensor, w_freq: torch.Tensor, stride: int = 1, padding: int = 0) -> torch.Tensor:
    """ConvolutionTheoremMatMul.frequency_conv1d"""
    return ConvolutionTheoremMatMul.frequency_conv1d(x, w_freq, stride, padding)
