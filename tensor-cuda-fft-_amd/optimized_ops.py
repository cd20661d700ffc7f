"""Mirror of `fft_tensor.optimized_ops` (reference fft_tensor/optimized_ops.py): OptimizedFrequencyOps (fast_topk_sparse
:27-43, optimized_sparse_fft :46-70, optimized_sparse_ifft :73-96, fast_frequency_matmul :99-144, fast_frequency_conv1d
:147-200, fast_frequency_conv2d :203-265) and ProductionFrequencyLinear (:268-346).  Names, arguments and defaults are the
reference's; its benchmark function and prints are not mirrored.

The hot path is the large-kernel, multi-channel FFT convolution.  Per frequency bin the reference forms
`(x_freq.unsqueeze(1) * w_freq.unsqueeze(0)).sum(dim=2)`, a materialised (B, C_out, C_in, n_fft) complex product; here it is
functional.bin_contract, one native launch that reads the weight spectrum once (csrc/smx_fconv.hip), between the package's
own differentiable transforms (functional.rfft / irfft / seq_fft) -- channels stay innermost from the first transform to
the last, and the one-sided spectrum of the real input halves the bins.  The top-k selection runs on
functional.sparsify_topk.  Off a ROCm device every member runs the reference's op sequence on torch."""
from typing import Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import functional as _fn
from .frequency_ops import ifft_last_real

_SMALL_K1 = 64                 # the reference's crossovers: kernels up to this size go to F.conv1d ...
_SMALL_K2 = 7                  # ... and up to this size on BOTH axes to F.conv2d
_MAX_NATIVE_FFT = 1 << 16      # transform lengths the native convolution path takes (powers of two up to this one)


def _next_pow2(n: int) -> int:
    """the reference's expression for its transform length"""
    return 2 ** int(np.ceil(np.log2(n)))


def _conv_native(x: torch.Tensor, w: torch.Tensor, *n_fft: int) -> bool:
    return (x.is_cuda and w.device == x.device and x.dtype == torch.float32 and w.dtype == torch.float32
            and x.numel() > 0 and w.numel() > 0 and all(2 <= n <= _MAX_NATIVE_FFT for n in n_fft))


def _ifft_seq(z: torch.Tensor) -> torch.Tensor:
    """torch.fft.ifft(z, dim=1) of a (B, N, D) complex64 tensor on the native sequence transform"""
    return _fn.seq_fft(z.conj()).conj() / z.shape[1]


class OptimizedFrequencyOps:
    @staticmethod
    def fast_topk_sparse(data: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(values, indices): the k elements of the flattened `data` that are largest in magnitude, in descending order
        of magnitude, and their int64 flat indices -- torch.topk(|data.flatten()|, k) and a gather, as in the reference
        (which compiles that with torch.jit.script; this is a plain function).
        For a complex64 tensor on a ROCm device that does not require grad the selection is functional.sparsify_topk(k=k)
        (an exact radix select, no sort of the whole tensor) followed by a sort of only its m >= k survivors by
        torch.abs; membership can differ from the reference only at a tie at the threshold (sparsify_topk compares
        fl(re re + im im), torch.topk compares torch.abs)."""
        flat = data.flatten()
        n = flat.numel()
        native = (flat.is_cuda and flat.dtype == torch.complex64 and not flat.requires_grad and 1 <= k <= n
                  and _fn.topk_supported(n))
        if not native:
            _, indices = torch.topk(torch.abs(flat), k)
            return flat[indices], indices
        coeffs, idx = _fn.sparsify_topk(flat, k=int(k))
        order = torch.argsort(torch.abs(coeffs), descending=True, stable=True)[:k]
        return coeffs[order], idx[order]

    @staticmethod
    def optimized_sparse_fft(spatial_data: torch.Tensor, sparsity: float,
                             return_indices: bool = True) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """fftn of `spatial_data` over all axes, then fast_topk_sparse with k = max(1, int(numel * sparsity)): the kept
        coefficients in descending order of magnitude, with their flat indices when return_indices.  On a ROCm device a
        float32 or complex64 input is transformed by functional.fftn (the native sequence transform, axis by axis);
        everything else by torch.fft.fftn."""
        if spatial_data.is_cuda and spatial_data.dtype in (torch.float32, torch.complex64) and spatial_data.numel() > 0 \
                and not spatial_data.requires_grad:
            freq = _fn.fftn(spatial_data) if spatial_data.is_complex() else _fn.fftn_real(spatial_data)
        else:
            freq = torch.fft.fftn(spatial_data)
        k = max(1, int(freq.numel() * sparsity))
        coeffs, indices = OptimizedFrequencyOps.fast_topk_sparse(freq, k)
        return (coeffs, indices) if return_indices else coeffs

    @staticmethod
    def optimized_sparse_ifft(sparse_coeffs: torch.Tensor, indices: torch.Tensor, output_shape: Tuple[int, ...],
                              device: str = 'cuda') -> torch.Tensor:
        """The real part of ifftn of the complex64 tensor of `output_shape` that is zero except flat[indices] =
        sparse_coeffs.  The indices arrive in magnitude order (fast_topk_sparse), not ascending, so the dense spectrum is
        built with zeros + index_put_ (functional.sparse_scatter's general branch): sorting the m pairs by index for the
        one-launch native scatter would cost a sort and two gathers to save one fill, and would pick another winner
        than index_put_ where an index repeats.  The inverse transform is functional.ifftn on a ROCm device."""
        coeffs = sparse_coeffs.to(device=device, dtype=torch.complex64)
        full = _fn.sparse_scatter(coeffs, indices.to(device=coeffs.device, dtype=torch.int64), tuple(output_shape))
        if full.is_cuda and full.numel() > 0 and not full.requires_grad:
            return _fn.ifftn_real(full)
        return torch.fft.ifftn(full).real

    @staticmethod
    def fast_frequency_matmul(x: torch.Tensor, w_freq: torch.Tensor, block_size: Optional[int] = None) -> torch.Tensor:
        """x (B, M, K) times the real part of the inverse transform of w_freq (K, N) along its LAST axis, (B, M, N).  A
        weight below 100 MB as float32, or block_size None, is inverted whole; otherwise block_size columns at a time
        (each block of spectrum columns inverted on its own: as in the reference, the blocks are NOT the columns of the
        whole inverse, so the two branches differ).  The inverse is the helper of FrequencyMatMul.circulant_matmul."""
        B, M, K = x.shape
        K2, N = w_freq.shape
        assert K == K2, f"Dimension mismatch: {K} != {K2}"
        matrix_size_mb = (K * N * 4) / (1024 ** 2)
        if matrix_size_mb < 100 or block_size is None:
            return torch.matmul(x, ifft_last_real(w_freq))
        output = torch.zeros(B, M, N, device=x.device, dtype=x.dtype)
        for n_start in range(0, N, block_size):
            n_end = min(n_start + block_size, N)
            output[:, :, n_start:n_end] = torch.matmul(x, ifft_last_real(w_freq[:, n_start:n_end]))
        return output

    @staticmethod
    def fast_frequency_conv1d(x: torch.Tensor, w: torch.Tensor, stride: int = 1, padding: int = 0) -> torch.Tensor:
        """x (B, C_in, L), w (C_out, C_in, K).  The reference's two branches compute DIFFERENT things, mirrored as they
        are:
          K <= 64: F.conv1d(x, w, stride=stride, padding=padding), a cross-correlation.
          K > 64:  with L' = L + 2 padding, the first L' - K + 1 samples, every stride-th, of the full LINEAR CONVOLUTION
                   y[b, o, n] = sum_c sum_k x_pad[b, c, n - k] w[o, c, k]   (x_pad zero before its first sample)
                   -- not F.conv1d's cross-correlation and not its "valid" region: the reference slices the circular
                   product of the zero-padded transforms from sample 0.  In torch terms:
                   F.conv1d(x_pad, w.flip(-1), padding=K - 1)[..., :L' - K + 1][..., ::stride].
        The K > 64 branch is native for float32 operands on a ROCm device with n_fft = 2 ** ceil(log2(L' + K - 1)) up to
        65536: x as (B, L', C_in) and w as (1, K, C_in C_out) go through functional.rfft (n = n_fft), the n_fft / 2 + 1 bins
        through functional.bin_contract, the result through functional.irfft (rows = L' - K + 1).  It is differentiable
        in x and w through those Functions.  Anything else runs the reference's op sequence on torch.fft (full-length
        complex transforms and the materialised (B, C_out, C_in, n_fft) product)."""
        B, C_in, L = x.shape
        C_out, C_in2, K = w.shape
        if K <= _SMALL_K1:
            return F.conv1d(x, w, stride=stride, padding=padding)
        if padding > 0:
            x = F.pad(x, (padding, padding))
            L = L + 2 * padding
        n_fft = _next_pow2(L + K - 1)
        valid = L - K + 1
        if valid >= 1 and C_in == C_in2 and _conv_native(x, w, n_fft):
            xs = _fn.rfft(x.transpose(1, 2), n=n_fft)                                            # (B, F, C_in)
            ws = _fn.rfft(w.permute(2, 1, 0).reshape(1, K, C_in * C_out), n=n_fft)               # (1, F, C_in C_out)
            ys = _fn.bin_contract(xs, ws.reshape(-1, C_in, C_out))                                  # (B, F, C_out)
            y = _fn.irfft(ys, n=n_fft, rows=valid).transpose(1, 2)                               # (B, C_out, valid)
        else:
            x_freq = torch.fft.fft(F.pad(x, (0, n_fft - L)), dim=-1)
            w_freq = torch.fft.fft(F.pad(w, (0, n_fft - K)), dim=-1)
            y_freq = (x_freq.unsqueeze(1) * w_freq.unsqueeze(0)).sum(dim=2)
            y = torch.fft.ifft(y_freq, dim=-1).real[:, :, :valid]
        if stride > 1:
            y = y[:, :, ::stride]
        return y

    @staticmethod
    def fast_frequency_conv2d(x: torch.Tensor, w: torch.Tensor, stride: Union[int, Tuple[int, int]] = 1,
                              padding: Union[int, Tuple[int, int]] = 0) -> torch.Tensor:
        """x (B, C_in, H, W), w (C_out, C_in, Kh, Kw).  Kh <= 7 and Kw <= 7: F.conv2d(x, w, stride, padding).  Otherwise
        (as in fast_frequency_conv1d, and just as different from the other branch) the top-left (H' - Kh + 1, W' - Kw + 1)
        corner, strided, of the full 2-D linear convolution of the padded input with w:
        F.conv2d(x_pad, w.flip(-2, -1), padding=(Kh - 1, Kw - 1))[..., :H' - Kh + 1, :W' - Kw + 1].
        Native for float32 operands on a ROCm device with both transform lengths (powers of two) up to 65536: the REAL
        transform (functional.rfft, fft_h / 2 + 1 bins) runs along H on x as (B, H', W' C_in), the complex one
        (functional.seq_fft, zero-padded to fft_w) along W, functional.bin_contract over the P = (fft_h / 2 + 1) fft_w
        bins, then conj(seq_fft(conj .)) / fft_w and functional.irfft back; differentiable in x and w.  The layout
        copies around the transforms (NCHW <-> channels-last, the zero-padding along W) are torch ops."""
        B, C_in, H, W = x.shape
        C_out, C_in2, Kh, Kw = w.shape
        if isinstance(stride, int):
            stride = (stride, stride)
        if isinstance(padding, int):
            padding = (padding, padding)
        if Kh <= _SMALL_K2 and Kw <= _SMALL_K2:
            return F.conv2d(x, w, stride=stride, padding=padding)
        if padding[0] > 0 or padding[1] > 0:
            x = F.pad(x, (padding[1], padding[1], padding[0], padding[0]))
            H = H + 2 * padding[0]
            W = W + 2 * padding[1]
        fft_h = _next_pow2(H + Kh - 1)
        fft_w = _next_pow2(W + Kw - 1)
        valid_h = H - Kh + 1
        valid_w = W - Kw + 1
        if valid_h >= 1 and valid_w >= 1 and C_in == C_in2 and _conv_native(x, w, fft_h, fft_w):
            Fh = fft_h // 2 + 1
            xs = _fn.rfft(x.permute(0, 2, 3, 1).reshape(B, H, W * C_in), n=fft_h)                # (B, Fh, W C_in)
            xs = _fn.seq_fft(F.pad(xs.reshape(B * Fh, W, C_in), (0, 0, 0, fft_w - W)))              # (B Fh, fft_w, C_in)
            ws = _fn.rfft(w.permute(2, 3, 1, 0).reshape(1, Kh, Kw * C_in * C_out), n=fft_h)      # (1, Fh, Kw C_in C_out)
            ws = _fn.seq_fft(F.pad(ws.reshape(Fh, Kw, C_in * C_out), (0, 0, 0, fft_w - Kw)))        # (Fh, fft_w, C_in C_out)
            ys = _fn.bin_contract(xs.reshape(B, Fh * fft_w, C_in), ws.reshape(Fh * fft_w, C_in, C_out))
            ys = _ifft_seq(ys.reshape(B * Fh, fft_w, C_out))[:, :valid_w]                           # (B Fh, valid_w, C_out)
            y = _fn.irfft(ys.reshape(B, Fh, valid_w * C_out), n=fft_h, rows=valid_h)             # (B, valid_h, valid_w C_out)
            y = y.reshape(B, valid_h, valid_w, C_out).permute(0, 3, 1, 2)
        else:
            x_freq = torch.fft.fft2(F.pad(x, (0, fft_w - W, 0, fft_h - H)), dim=(-2, -1))
            w_freq = torch.fft.fft2(F.pad(w, (0, fft_w - Kw, 0, fft_h - Kh)), dim=(-2, -1))
            y_freq = (x_freq.unsqueeze(1) * w_freq.unsqueeze(0)).sum(dim=2)
            y = torch.fft.ifft2(y_freq, dim=(-2, -1)).real[:, :, :valid_h, :valid_w]
        if stride[0] > 1 or stride[1] > 1:
            y = y[:, :, ::stride[0], ::stride[1]]
        return y


class ProductionFrequencyLinear(torch.nn.Module):
    """The reference's ProductionFrequencyLinear: a linear layer whose weight is kept as the (out_features, in_features)
    complex spectrum of its rows with all but the k = max(1, int(in_features * sparsity)) largest bins of each row zeroed
    at construction; forward is F.linear(x, Re(ifft(weight_freq, dim=-1)), bias).  State: weight_freq, bias,
    weight_indices (a reference state_dict loads with strict=True).  The initial draw is made on the CPU exactly as the
    reference makes it, so a seed gives the same layer; the reference's per-row loop that copies the kept bins is one
    gather / scatter.  In eval mode the materialised weight is cached until invalidate_cache(), as in the reference.
    On a ROCm device the inverse transform of a complex64 weight_freq runs without an FFT library: where a gradient can be
    asked for (grad enabled and weight_freq requires grad) it is the package's differentiable sequence transform
    (functional.seq_fft), so forward is differentiable in weight_freq; otherwise (no_grad, a frozen weight) it is
    frequency_ops.ifft_last_real, one launch of the native row transform where the length has one."""

    def __init__(self, in_features: int, out_features: int, sparsity: float = 0.05, bias: bool = True):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.sparsity = sparsity
        weight = torch.randn(out_features, in_features) * np.sqrt(2.0 / in_features)
        weight_freq = torch.fft.fft(weight, dim=-1)
        k = max(1, int(in_features * sparsity))
        _, indices = torch.topk(torch.abs(weight_freq), k, dim=-1)
        self.register_buffer('weight_indices', indices)
        sparse_freq = torch.zeros_like(weight_freq).scatter_(1, indices, weight_freq.gather(1, indices))
        self.weight_freq = torch.nn.Parameter(sparse_freq)
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(out_features))
        else:
            self.register_parameter('bias', None)
        self._weight_cache = None
        self._cache_valid = False

    def _materialize_weights(self) -> torch.Tensor:
        if self._cache_valid and self._weight_cache is not None:
            return self._weight_cache
        wf = self.weight_freq
        if wf.is_cuda and wf.dtype == torch.complex64 and wf.numel() > 0 and not (torch.is_grad_enabled() and wf.requires_grad):
            weight = ifft_last_real(wf.detach())                  # nothing to differentiate: one native row launch
        elif wf.is_cuda and wf.dtype == torch.complex64 and wf.numel() > 0:
            weight = _fn.seq_fft(wf.conj().unsqueeze(-1)).squeeze(-1).real / wf.shape[-1]    # Re(conj(s) / n) = Re(s) / n
        else:
            weight = torch.fft.ifft(wf, dim=-1).real
        if not self.training:
            self._weight_cache = weight
            self._cache_valid = True
        return weight

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return F.linear(x, self._materialize_weights(), self.bias)

    def invalidate_cache(self):
        """Call after weight updates during training."""
        self._cache_valid = False
