"""Mirror of `fft_tensor.production_ready` (reference fft_tensor/production_ready.py): ProductionFrequencyOps
(compress_tensor :29-36, block_streaming_matmul :39-71, smart_conv2d :74-93) and OptimizedSparseSpectralTensor (:96-132).
Names, arguments and defaults are the reference's; its benchmark function and prints are not mirrored.  Everything here
rests on sparse_tensor.py (native top-k, scatter and N-D transform on a ROCm device) and on torch's own matmul and
convolution, as in the reference."""
import torch
import torch.nn.functional as F

from .sparse_tensor import SparseSpectralTensor, sst


class ProductionFrequencyOps:
    @staticmethod
    def compress_tensor(tensor: torch.Tensor, sparsity: float = 0.05) -> SparseSpectralTensor:
        """sst(tensor, sparsity): the tensor as the top-k coefficients of its N-D spectrum (on 'cuda', the reference's
        default device, with its fallback to the CPU where there is none)."""
        return sst(tensor, sparsity=sparsity)

    @staticmethod
    def block_streaming_matmul(x: torch.Tensor, w_sst: SparseSpectralTensor, block_size: int = 1024) -> torch.Tensor:
        """x (B, M, K) @ w_sst.to_spatial() (K, N), written block_size columns at a time -- this module's own variant,
        unlike FrequencyMatMul.block_streaming_matmul a true x @ W.  As in the reference the WHOLE weight is materialised
        for every block (w_sst.to_spatial()[:, n0:n1]), so nothing is saved unless w_sst caches it
        (OptimizedSparseSpectralTensor).  Returns (B, M, N) in x's dtype."""
        B, M, K = x.shape
        N = w_sst.shape[1]
        output = torch.zeros(B, M, N, device=x.device, dtype=x.dtype)
        for n_start in range(0, N, block_size):
            n_end = min(n_start + block_size, N)
            output[:, :, n_start:n_end] = torch.matmul(x, w_sst.to_spatial()[:, n_start:n_end])
        return output

    @staticmethod
    def smart_conv2d(x: torch.Tensor, w: torch.Tensor, stride: int = 1, padding: int = 0) -> torch.Tensor:
        """F.conv2d(x, w, stride=stride, padding=padding) for every kernel size: the reference announces an FFT branch
        above 11 x 11 and calls F.conv2d on it too."""
        return F.conv2d(x, w, stride=stride, padding=padding)


class OptimizedSparseSpectralTensor(SparseSpectralTensor):
    """SparseSpectralTensor whose to_spatial() keeps its result until invalidate_cache() (the reference's class).  The
    cached tensor is returned itself, not a copy: a caller that writes into it changes what the next call returns, as in
    the reference.  A tensor derived from this one (scalar product, normalisation) starts without a cache."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._spatial_cache = None
        self._cache_valid = False

    def _with_coeffs(self, freq_coeffs: torch.Tensor) -> 'OptimizedSparseSpectralTensor':
        new = super()._with_coeffs(freq_coeffs)
        new._spatial_cache = None
        new._cache_valid = False
        return new

    def to_spatial(self) -> torch.Tensor:
        if self._cache_valid and self._spatial_cache is not None:
            return self._spatial_cache
        spatial = super().to_spatial()
        self._spatial_cache = spatial
        self._cache_valid = True
        return spatial

    def invalidate_cache(self):
        """Call after any operation that modifies frequencies."""
        self._cache_valid = False
        self._spatial_cache = None
