"""Mirror of `fft_tensor.frequency_ops` (reference fft_tensor/frequency_ops.py): FrequencyMatMul (circulant_matmul :31-72,
block_streaming_matmul :75-131 on a SparseSpectralTensor weight, sparse_tensor.py), FrequencyAttention
(frequency_attention :147-185 on the native attention of functional.py, fnet_attention :188-204 on the native sequence
transform), ComplexSemanticEmbedding (:207-310), FrequencyTransformerLayer (:313-363), frequency_relu (:367-381) and
frequency_layernorm (:384-401, native).  Names, arguments and defaults are the reference's.  The hot paths -- the attention
and the layernorm -- are HIP kernels (csrc/smx_freq.hip), forward only: operands that require grad run the reference's own
torch ops.  The four complex GEMMs of the layer stay torch.matmul."""
from __future__ import annotations

import torch

from . import functional as _fn
from .functional import seq_fft
from .sparse_tensor import SparseSpectralTensor


def ifft_last_real(w_freq: torch.Tensor) -> torch.Tensor:
    """torch.fft.ifft(w_freq, dim=-1).real of a 2-D weight.  On a ROCm device the inverse transform of a complex64 weight
    that does not require grad is ONE launch of the native row transform where functional.rowfft_supported(n):
    conjugated on the way in, scaled by 1 / n, the real part alone written (Re(ifft w) = Re(F conj w) / n).  Other
    lengths run the package's sequence transform, ifft(w) = conj(fft(conj w)) / n as functional.ifftn does it; CPU
    tensors (and every other weight) use torch.fft."""
    if w_freq.is_cuda and w_freq.dtype == torch.complex64 and not w_freq.requires_grad and w_freq.numel() > 0:
        if _fn._row_native(w_freq):
            return _fn.row_fft_raw(w_freq, conj_in=True, real_out=True, scale=1.0 / w_freq.shape[-1])
        spec = _fn.seq_fft_raw(w_freq.conj().resolve_conj().unsqueeze(-1)).squeeze(-1)
        return spec.real / w_freq.shape[-1]              # Re(conj(s) / n) = Re(s) / n
    return torch.fft.ifft(w_freq, dim=-1).real


class FrequencyMatMul:
    @staticmethod
    def circulant_matmul(x: torch.Tensor, w_freq: torch.Tensor) -> torch.Tensor:
        """The reference's circulant_matmul as it is (it calls itself deprecated: not a circulant product but a plain
        matmul with the inverse transform of the weight's LAST axis): x (B, M, K); w_freq (D_out, D_in) with D_in == K
        gives x @ ifft(w_freq).real.T, (B, M, D_out); otherwise w_freq (K, N) gives x @ ifft(w_freq).real, (B, M, N).
        On a ROCm device the inverse transform of a complex64 weight that does not require grad is the package's own
        sequence transform, ifft(w) = conj(fft(conj w)) / n as functional.ifftn does it; CPU tensors (and every other
        weight) use torch.fft."""
        B, M, K = x.shape
        if len(w_freq.shape) == 2:
            D_out, D_in = w_freq.shape
            if D_in != K and D_out != K:
                raise ValueError(f"Dimension mismatch: x has {K}, w_freq is {w_freq.shape}")
            w_spatial = ifft_last_real(w_freq)
            return torch.matmul(x, w_spatial.T if D_in == K else w_spatial)
        raise ValueError(f"Unexpected w_freq shape: {w_freq.shape}")

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
    def frequency_attention(q_freq: torch.Tensor, k_freq: torch.Tensor, v_freq: torch.Tensor,
                            temperature: float = 1.0) -> torch.Tensor:
        """softmax_n(mean_d |q conj(k)| / temperature)[..., None] * v for complex (B, H, N, D): functional.frequency_attention
        (native and forward-only on a ROCm device; the reference's torch ops for CPU tensors and operands that require
        grad)."""
        return _fn.frequency_attention(q_freq, k_freq, v_freq, temperature)

    @staticmethod
    def fnet_attention(x_freq: torch.Tensor) -> torch.Tensor:
        """torch.fft.fft(x_freq, dim=1) for complex64 (B, N, D) on a ROCm device."""
        return seq_fft(x_freq)


class ComplexSemanticEmbedding:
    """The reference's complex-valued embedding table: `freq_embeddings` (vocab_size, embed_dim) complex64, a plain
    tensor, initialised by the reference's sequence -- randn * 0.02, times exp(-j / 10) along the embedding axis, times
    exp(i randn).  The values come from the generator of `device`, so on a ROCm device they are not the numbers the
    reference draws on its device for the same seed (assign `freq_embeddings` to carry a table over)."""

    def __init__(self, vocab_size: int, embed_dim: int, device: str = 'cuda'):
        self.vocab_size, self.embed_dim, self.device = vocab_size, embed_dim, device
        # two draws from the device's generator, in the reference's order: the complex table, then one real angle per entry
        table = 0.02 * torch.randn(vocab_size, embed_dim, dtype=torch.complex64, device=device)
        falloff = torch.exp(torch.arange(embed_dim, device=device) / -10.0)       # column j scaled by e^(-j / 10)
        angles = torch.randn(vocab_size, embed_dim, device=device)
        self.freq_embeddings = (table * falloff) * torch.exp(1j * angles)          # ... and turned by its angle

    def lookup(self, token_ids: torch.Tensor) -> torch.Tensor:
        """freq_embeddings[token_ids]: (B, N) ids -> (B, N, D) complex"""
        return self.freq_embeddings[token_ids]

    def semantic_similarity(self, freq1: torch.Tensor, freq2: torch.Tensor) -> torch.Tensor:
        """|sum_d freq1 conj(freq2)|: (B, D), (B, D) -> (B,) real"""
        return torch.abs(torch.sum(freq1 * torch.conj(freq2), dim=-1))

    def phase_relationship(self, freq1: torch.Tensor, freq2: torch.Tensor) -> torch.Tensor:
        """angle(freq1 / (freq2 + 1e-8))"""
        return torch.angle(freq1 / (freq2 + 1e-8))


class FrequencyTransformerLayer:
    """The reference's frequency-domain transformer layer: four plain complex64 (d_model, d_model) weights
    (`q_proj_freq`, `k_proj_freq`, `v_proj_freq`, `o_proj_freq`, randn * 0.02 from the generator of `device`; they may be
    reassigned between calls -- nothing derived from them is kept), and
        forward(x) = attention(heads(x @ Wq), heads(x @ Wk), heads(x @ Wv)) merged back to (B, N, D), @ Wo.
    The four GEMMs are torch.matmul.  On a ROCm device the attention reads the (B, N, H, hd) projections through their
    (B, H, N, hd) views and writes the merged (B, N, D) result directly: the reference's three head transposes and its
    `.contiguous()` copy do not exist here."""

    def __init__(self, d_model: int, n_heads: int, device: str = 'cuda'):
        self.d_model = d_model
        self.n_heads = n_heads
        self.head_dim = d_model // n_heads
        self.device = device
        self.q_proj_freq = torch.randn(d_model, d_model, dtype=torch.complex64, device=device) * 0.02
        self.k_proj_freq = torch.randn(d_model, d_model, dtype=torch.complex64, device=device) * 0.02
        self.v_proj_freq = torch.randn(d_model, d_model, dtype=torch.complex64, device=device) * 0.02
        self.o_proj_freq = torch.randn(d_model, d_model, dtype=torch.complex64, device=device) * 0.02

    def forward(self, x_freq: torch.Tensor) -> torch.Tensor:
        """x_freq (B, N, D) complex -> (B, N, D) complex"""
        B, N, D = x_freq.shape
        heads = lambda t: t.view(B, N, self.n_heads, self.head_dim).transpose(1, 2)
        attn = _fn.frequency_attention(heads(x_freq @ self.q_proj_freq), heads(x_freq @ self.k_proj_freq),
                                       heads(x_freq @ self.v_proj_freq), merge_heads=True)
        return attn.view(B, N, D) @ self.o_proj_freq


def frequency_relu(x_freq: torch.Tensor) -> torch.Tensor:
    """The reference's frequency_relu in plain torch: relu(|z|) * exp(i angle(z)).  A magnitude is never negative, so
    this is the identity up to rounding (z == 0 stays 0); it is mirrored for the name, and has no kernel."""
    return torch.relu(torch.abs(x_freq)) * torch.exp(1j * torch.angle(x_freq))


def frequency_layernorm(x_freq: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """(|z| - mean) / (std + eps) * exp(i angle(z)) over the last axis: functional.frequency_layernorm (native and
    forward-only on a ROCm device; the reference's torch ops for CPU tensors and inputs that require grad)."""
    return _fn.frequency_layernorm(x_freq, eps)
