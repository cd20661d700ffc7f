"""Mirror of the three functions of `fft_tensor.ops` that work in the reference (fft_tensor/ops.py:29-105):
spectral_pool, spectral_normalize and spectral_activation on SparseSpectralTensor.

Left out, because they cannot run in the reference either or rest on parts that are: spectral_conv (calls a method
`_hadamard` that does not exist), implicit_matmul (its streaming branch raises NameError: numpy is never imported),
ImplicitWeights and spectral_backward.  Nothing here is differentiable, as in the reference."""
from __future__ import annotations

import torch

from .sparse_tensor import SparseSpectralTensor, sst


def spectral_pool(input_sst: SparseSpectralTensor, kernel_size: int = 2, mode: str = 'max') -> SparseSpectralTensor:
    """max_pool2d / avg_pool2d of the materialised 2-D tensor, sparsified again at
    max(0.01, min(sparsity / kernel_size**2, sparsity)) -- the reference's route; like it, 2-D tensors only."""
    if mode not in ('max', 'avg'):
        raise ValueError(f"Unknown pooling mode: {mode}")
    new_sparsity = max(0.01, min(input_sst.sparsity / (kernel_size ** 2), input_sst.sparsity))
    spatial = input_sst.to_spatial().unsqueeze(0).unsqueeze(0)
    pool = torch.nn.functional.max_pool2d if mode == 'max' else torch.nn.functional.avg_pool2d
    return sst(pool(spatial, kernel_size=kernel_size).squeeze(), sparsity=new_sparsity, device=input_sst.device)


def spectral_normalize(input_sst: SparseSpectralTensor, eps: float = 1e-5) -> SparseSpectralTensor:
    """the coefficients divided by (the sum of their magnitudes + eps); positions unchanged, nothing materialised"""
    norm = torch.abs(input_sst.freq_coeffs).sum() + eps
    return input_sst._with_coeffs(input_sst.freq_coeffs / norm)


_ACTIVATIONS = {'relu': torch.relu, 'gelu': torch.nn.functional.gelu, 'silu': torch.nn.functional.silu,
                'tanh': torch.tanh}


def spectral_activation(input_sst: SparseSpectralTensor, activation: str = 'relu') -> SparseSpectralTensor:
    """materialise, apply 'relu' / 'gelu' / 'silu' / 'tanh', sparsify again at the same sparsity"""
    if activation not in _ACTIVATIONS:
        raise ValueError(f"Unknown activation: {activation}")
    return sst(_ACTIVATIONS[activation](input_sst.to_spatial()), sparsity=input_sst.sparsity, device=input_sst.device)
