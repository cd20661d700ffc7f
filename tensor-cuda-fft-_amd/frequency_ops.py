"""Mirror of the members of `fft_tensor.frequency_ops` that this package can serve:
`FrequencyAttention.fnet_attention` (reference fft_tensor/frequency_ops.py:188-204) -- a full complex FFT along the
sequence axis of a complex (B, N, D) tensor, here the native transform (functional.seq_fft) -- and
`FrequencyMatMul.block_streaming_matmul` (:75-131) on a SparseSpectralTensor weight (sparse_tensor.py).
The rest of that module (circulant_matmul, which the reference itself marks deprecated, ComplexSemanticEmbedding, ...)
is out of scope."""
from __future__ import annotations

import torch

from .functional import seq_fft
from .sparse_tensor import SparseSpectralTensor


class FrequencyMatMul:
    @staticmethod
    def block_streaming_matmul(x: torch.Tensor, w_sst: SparseSpectralTensor, block_size: int = 512) -> torch.Tensor:
        """What the reference computes, block by block of `block_size` columns n0 <= c < n1 of the (K, N) weight:
        the stored coefficients whose FREQUENCY column index lies in the block become a (K, n1 - n0) sparse tensor of
        their own (column index minus n0), that tensor is materialised (a K x (n1 - n0) inverse transform) and
        output[:, :, n0:n1] = x @ it; a block without coefficients stays zero.

        The reference's docstring calls this x @ W with only block_size columns of W in memory.  It is not: a block of
        columns of the SPECTRUM is not the spectrum of a block of columns of W, so for block_size < N the result
        differs from x @ w_sst.to_spatial(); only block_size >= N gives that product.  The arithmetic is mirrored as it
        is (results agree with the reference's); the memory claim does hold -- one K x block_size tensor at a time.

        x: (B, M, K) real; returns (B, M, N) in x's dtype.  Not differentiable."""
        B, M, K = x.shape
        N = w_sst.shape[1]
        output = torch.zeros(B, M, N, device=x.device, dtype=x.dtype)
        for n_start in range(0, N, block_size):
            n_end = min(n_start + block_size, N)
            mask = (w_sst.indices[:, 1] >= n_start) & (w_sst.indices[:, 1] < n_end)
            block_coeffs = w_sst.freq_coeffs[mask]
            if len(block_coeffs) > 0:
                shift = torch.tensor([0, n_start], device=w_sst.indices.device)
                block = SparseSpectralTensor(freq_coeffs=block_coeffs, indices=w_sst.indices[mask] - shift,
                                             shape=(K, n_end - n_start), sparsity=w_sst.sparsity, device=w_sst.device,
                                             dtype=w_sst.dtype, use_cuda_backend=w_sst.use_cuda)
                output[:, :, n_start:n_end] = torch.matmul(x, block.to_spatial())
        return output


class FrequencyAttention:
    @staticmethod
    def fnet_attention(x_freq: torch.Tensor) -> torch.Tensor:
        """torch.fft.fft(x_freq, dim=1) for complex64 (B, N, D) on a ROCm device."""
        return seq_fft(x_freq)
