"""Mirror of `fft_tensor.tensor` (reference fft_tensor/tensor.py): SparseSpectralTensor, MemoryManager, sst, zeros_sst,
randn_sst -- a tensor kept as the top-k coefficients of its N-D spectrum.

The reference declares a native extension for the four steps of this type (fft_tensor/setup.py:20-49: sparsify_topk,
sparse_scatter, fft_forward, fft_inverse) whose sources were never written, so every reference user runs its torch
fallback.  Here a tensor on a ROCm device is served by functional.sparsify_topk / sparse_scatter (csrc/smx_sst.hip) and by
functional.fftn / ifftn (the native sequence transform, axis by axis); `use_cuda` says so.  A CPU tensor, and a device
tensor built with use_cuda_backend=False, runs the same definitions with torch ops.

Deliberate differences from the reference: no gc.collect() / empty_cache() per construction and
materialisation; no print or warning at import; membership at an exact magnitude tie follows the squared key of
functional.sparsify_topk, not torch.abs; MemoryManager holds weak references, so it counts the tensors that are alive
instead of keeping every tensor alive until clear_all().

Nothing here is differentiable, as in the reference."""
from __future__ import annotations

import warnings
import weakref
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import functional as F


def _resolve_device(device):
    """the reference's fallback: 'cuda' without a device becomes 'cpu', with its warning"""
    if torch.device(device).type == "cuda" and not torch.cuda.is_available():
        warnings.warn("CUDA not available, falling back to CPU")
        return "cpu"
    return device


class SparseSpectralTensor:
    """A real tensor of `shape` stored as the `freq_coeffs` (m,) complex64 of its N-D DFT at the positions `indices`
    (m, ndim) int64 -- the k = max(1, int(numel * sparsity)) largest magnitudes and everything that ties with the k-th.

    >>> w = SparseSpectralTensor(data=torch.randn(1000, 1000, device='cuda'), sparsity=0.05)
    >>> w.compress_ratio(), w.to_spatial().shape

    Constructor arguments, attributes and methods are the reference's (fft_tensor/tensor.py:45-297)."""

    def __init__(self, data: Optional[torch.Tensor] = None, freq_coeffs: Optional[torch.Tensor] = None,
                 indices: Optional[torch.Tensor] = None, shape: Optional[Tuple[int, ...]] = None,
                 sparsity: float = 0.05, device: str = 'cuda', dtype: torch.dtype = torch.float32,
                 use_cuda_backend: bool = True):
        device = _resolve_device(device)
        self.device = device
        self.dtype = dtype
        self.sparsity = sparsity
        self.use_cuda = bool(use_cuda_backend) and torch.device(device).type == "cuda"
        if data is not None:
            self._from_spatial(data)
        elif freq_coeffs is not None and indices is not None:
            if shape is None:
                raise ValueError("shape required when providing freq_coeffs")
            self.freq_coeffs = freq_coeffs.to(device=device, dtype=torch.complex64)
            self.indices = indices.to(device=device, dtype=torch.long)
            self.shape = tuple(shape)
            self._flat, self._ascending = self._flatten_indices()
        else:
            raise ValueError("Must provide either data or (freq_coeffs, indices, shape)")
        self._register_memory()

    # ---- construction ---------------------------------------------------------------------------------------------------------
    def _from_spatial(self, data) -> None:
        if not isinstance(data, torch.Tensor):
            data = torch.tensor(data)
        self.shape = tuple(data.shape)
        with torch.no_grad():
            x = data.detach().to(device=self.device, dtype=self.dtype)
            if self.use_cuda and x.dtype == torch.float32:
                freq = F.fftn_real(x)                # the last axis reads the fp32 rows: no complex copy of the input
            else:
                z = x.to(torch.complex64)
                freq = F.fftn(z) if self.use_cuda else torch.fft.fftn(z)
            if self.use_cuda:
                self.freq_coeffs, flat = F.sparsify_topk(freq, self.sparsity)
            else:
                if freq.numel() == 0:
                    raise ValueError("SparseSpectralTensor: data is empty")
                flat_freq = freq.reshape(-1)
                self.freq_coeffs, flat = F._sparsify_torch(flat_freq, max(1, int(flat_freq.numel() * self.sparsity)))
        self.indices = self._flat_to_nd_indices(flat, self.shape)
        self._flat, self._ascending = flat, True

    def _flat_to_nd_indices(self, flat_indices: torch.Tensor, shape: Tuple[int, ...]) -> torch.Tensor:
        """(m,) flat -> (m, ndim), the reference's loop (fft_tensor/tensor.py:146-155)"""
        nd, remaining = [], flat_indices
        for dim_size in reversed(shape):
            nd.insert(0, remaining % dim_size)
            remaining = remaining // dim_size
        return torch.stack(nd, dim=1) if nd else flat_indices.new_zeros((flat_indices.numel(), 0))

    def _flatten_indices(self):
        """(flat indices, whether the native scatter may take them): computed once for a tensor built from
        (freq_coeffs, indices, shape) -- strictly ascending, every coordinate inside its axis.  One host read;
        construction is not hot."""
        idx = self.indices
        if idx.dim() == 1:                                      # the reference's scatter also takes flat indices
            flat, inside = idx, bool(((idx >= 0) & (idx < int(np.prod(self.shape)))).all())
        else:
            sizes = torch.tensor(self.shape, dtype=torch.long, device=idx.device)
            strides = torch.tensor([int(np.prod(self.shape[i + 1:])) for i in range(len(self.shape))], dtype=torch.long,
                                   device=idx.device)
            flat = (idx * strides).sum(dim=1)
            inside = bool(((idx >= 0) & (idx < sizes)).all())
        ascending = inside and bool((flat[1:] > flat[:-1]).all()) and flat.numel() == self.freq_coeffs.numel()
        return flat, ascending

    def _with_coeffs(self, freq_coeffs: torch.Tensor) -> 'SparseSpectralTensor':
        """the same positions with other coefficients: nothing is materialised, the index checks are not repeated"""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new.freq_coeffs = freq_coeffs.to(device=self.device, dtype=torch.complex64)
        new._register_memory()
        return new

    # ---- materialisation ------------------------------------------------------------------------------------------------------
    def to_spatial(self) -> torch.Tensor:
        """The dense real tensor of `shape` and `dtype`: scatter the coefficients into a zero spectrum, inverse N-D
        DFT, real part."""
        with torch.no_grad():
            if self.use_cuda and self._ascending:
                freq = F.sparse_scatter(self.freq_coeffs, self._flat, self.shape, assume_ascending=True)
            else:
                freq = self._scatter_pytorch()
            if self.use_cuda:
                return F.ifftn_real(freq).to(dtype=self.dtype)   # the last axis writes the real part alone
            return torch.fft.ifftn(freq).real.to(dtype=self.dtype)

    def _scatter_pytorch(self) -> torch.Tensor:
        freq = torch.zeros(self.shape, dtype=torch.complex64, device=self.device)
        if self.indices.dim() == 1:
            freq.flatten()[self.indices] = self.freq_coeffs
        else:
            freq[tuple(self.indices.t())] = self.freq_coeffs
        return freq

    # ---- arithmetic -------------------------------------------------------------------------------------------------------------
    def _from_result(self, spatial: torch.Tensor) -> 'SparseSpectralTensor':
        return SparseSpectralTensor(data=spatial, sparsity=self.sparsity, device=self.device,
                                    use_cuda_backend=self.use_cuda)

    def __add__(self, other: 'SparseSpectralTensor') -> 'SparseSpectralTensor':
        """materialise both, add, sparsify again (the reference's route)"""
        if self.shape != other.shape:
            raise ValueError(f"Shape mismatch: {self.shape} vs {other.shape}")
        return self._from_result(self.to_spatial() + other.to_spatial())

    def __mul__(self, other: Union['SparseSpectralTensor', float, int]) -> 'SparseSpectralTensor':
        """a scalar scales the coefficients (nothing is materialised); another tensor: the Hadamard product in space"""
        if isinstance(other, (int, float)):
            return self._with_coeffs(self.freq_coeffs * other)
        return self._from_result(self.to_spatial() * other.to_spatial())

    def __rmul__(self, other: Union[float, int]) -> 'SparseSpectralTensor':
        return self.__mul__(other)

    def matmul(self, other: 'SparseSpectralTensor') -> 'SparseSpectralTensor':
        """materialise both, torch.matmul, sparsify again (the reference's route)"""
        return self._from_result(torch.matmul(self.to_spatial(), other.to_spatial()))

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def compress_ratio(self) -> float:
        spatial_size = np.prod(self.shape)
        freq_size = len(self.freq_coeffs)
        return spatial_size / freq_size if freq_size > 0 else 0.0

    @torch.no_grad()
    def memory_mb(self) -> float:
        coeffs_bytes = self.freq_coeffs.element_size() * self.freq_coeffs.numel()
        indices_bytes = self.indices.element_size() * self.indices.numel()
        return (coeffs_bytes + indices_bytes) / (1024 ** 2)

    def _register_memory(self) -> None:
        MemoryManager.register(self)

    def __del__(self):
        try:
            MemoryManager.unregister(self)
        except Exception:
            pass                                                # interpreter shutdown

    def __repr__(self) -> str:
        return (f"SparseSpectralTensor(shape={self.shape}, "
                f"sparsity={self.sparsity:.3f}, "
                f"n_coeffs={len(self.freq_coeffs)}, "
                f"compression={self.compress_ratio():.1f}x, "
                f"memory={self.memory_mb():.2f}MB)")


class MemoryManager:
    """The reference's global tracker (fft_tensor/tensor.py:300-393): the sum of memory_mb() over the tensors that are
    alive, a limit (5000 MB by default) and a MemoryError when a new tensor passes it.  `_tensors` holds weak
    references."""
    _tensors: List["weakref.ref"] = []
    _max_memory_mb: int = 5000

    @classmethod
    def _alive(cls) -> list:
        live = [(r, r()) for r in cls._tensors]
        cls._tensors = [r for r, t in live if t is not None]
        return [t for _, t in live if t is not None]

    @classmethod
    def register(cls, tensor: SparseSpectralTensor) -> None:
        cls._tensors.append(weakref.ref(tensor))
        cls._check_memory()

    @classmethod
    def unregister(cls, tensor: SparseSpectralTensor) -> None:
        cls._tensors = [r for r in cls._tensors if r() is not None and r() is not tensor]

    @classmethod
    def total_memory_mb(cls) -> float:
        return sum(t.memory_mb() for t in cls._alive())

    @classmethod
    def _check_memory(cls) -> None:
        total = cls.total_memory_mb()
        if total > cls._max_memory_mb:
            raise MemoryError(
                f"SST memory limit exceeded: {total:.1f}MB / {cls._max_memory_mb}MB\n"
                f"Consider:\n"
                f"  1. Increasing sparsity\n"
                f"  2. Processing in smaller batches\n"
                f"  3. Calling MemoryManager.clear_all()")

    @classmethod
    def set_limit(cls, mb: int) -> None:
        if mb <= 0:
            raise ValueError("Memory limit must be positive")
        cls._max_memory_mb = mb

    @classmethod
    def clear_all(cls) -> None:
        """forget every tracked tensor (they stay valid; they no longer count)"""
        cls._tensors = []

    @classmethod
    def get_stats(cls) -> dict:
        total = cls.total_memory_mb()
        stats = {'n_tensors': len(cls._tensors), 'total_memory_mb': total, 'limit_mb': cls._max_memory_mb,
                 'utilization': total / cls._max_memory_mb}
        if torch.cuda.is_available():
            stats['cuda_allocated_mb'] = torch.cuda.memory_allocated() / (1024 ** 2)
            stats['cuda_reserved_mb'] = torch.cuda.memory_reserved() / (1024 ** 2)
        return stats


def sst(data: torch.Tensor, sparsity: float = 0.05, device: str = 'cuda') -> SparseSpectralTensor:
    """SparseSpectralTensor(data=data, sparsity=sparsity, device=device)"""
    return SparseSpectralTensor(data=data, sparsity=sparsity, device=device)


def zeros_sst(shape: Tuple[int, ...], sparsity: float = 0.05, device: str = 'cuda') -> SparseSpectralTensor:
    """of zeros: every coefficient ties at 0, so all of them are kept"""
    device = _resolve_device(device)
    return SparseSpectralTensor(data=torch.zeros(shape, device=device), sparsity=sparsity, device=device)


def randn_sst(shape: Tuple[int, ...], sparsity: float = 0.05, device: str = 'cuda') -> SparseSpectralTensor:
    """of standard normal values"""
    device = _resolve_device(device)
    return SparseSpectralTensor(data=torch.randn(shape, device=device), sparsity=sparsity, device=device)
