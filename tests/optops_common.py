"""Shared by tests/test_optops_cpu.py, tests/test_optops_gpu.py and tests/golden/make_golden_optops.py: the cases of
fft_tensor/optimized_ops.py and production_ready.py and their float64 / complex128 definitions (the yardsticks)."""
import numpy as np
import torch
import torch.nn.functional as F

# (B, Ci, Co, L, K, padding, stride): K > 64, the reference's FFT branch
CONV1D = [(2, 3, 5, 200, 65, 0, 1), (3, 7, 2, 300, 100, 4, 2), (9, 17, 33, 130, 129, 0, 1), (1, 1, 1, 65, 65, 0, 1)]
# (B, Ci, Co, H, W, Kh, Kw, padding, stride): Kh > 7 or Kw > 7
CONV2D = [(2, 3, 4, 20, 24, 9, 3, (0, 0), (1, 1)), (1, 2, 3, 16, 40, 3, 12, (1, 2), (2, 1)),
          (2, 5, 3, 33, 17, 8, 8, (0, 0), (1, 1))]
# n_fft = 8192: the four-step transform runs (GPU only; its inputs are drawn, not recorded)
CONV1D_FOURSTEP = (1, 2, 2, 3000, 1200, 0, 1)
SEED = 4321

MEMBERS = {
    "OptimizedFrequencyOps": ["fast_topk_sparse", "optimized_sparse_fft", "optimized_sparse_ifft", "fast_frequency_matmul",
                              "fast_frequency_conv1d", "fast_frequency_conv2d"],
    "ProductionFrequencyLinear": ["__init__", "forward", "invalidate_cache"],
    "ProductionFrequencyOps": ["compress_tensor", "block_streaming_matmul", "smart_conv2d"],
    "OptimizedSparseSpectralTensor": ["__init__", "to_spatial", "invalidate_cache"],
}


def conv1d_name(i):
    return "O%02d_conv1d_" % (i + 1) + "x".join(str(v) for v in CONV1D[i])


def conv2d_name(i):
    c = CONV2D[i]
    return "O%02d_conv2d_" % (i + 11) + "x".join(str(v) for v in c[:7])


def conv1d_inputs(case, seed=SEED):
    B, Ci, Co, L, K, _, _ = case
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Ci, L, generator=g), torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5


def conv2d_inputs(case, seed=SEED):
    B, Ci, Co, H, W, Kh, Kw, _, _ = case
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, Kh, Kw, generator=g) / (Ci * Kh * Kw) ** 0.5


def conv1d_def(x, w, stride=1, padding=0):
    """The K > 64 branch in float64: the first L' - K + 1 samples of the FULL linear convolution sum_k x[n - k] w[k]."""
    x, w = x.double(), w.double()
    K = w.shape[-1]
    x = F.pad(x, (padding, padding))
    valid = x.shape[-1] - K + 1
    return F.conv1d(x, w.flip(-1), padding=K - 1)[..., :valid][..., ::stride]


def conv2d_def(x, w, stride=(1, 1), padding=(0, 0)):
    x, w = x.double(), w.double()
    Kh, Kw = w.shape[-2:]
    x = F.pad(x, (padding[1], padding[1], padding[0], padding[0]))
    vh, vw = x.shape[-2] - Kh + 1, x.shape[-1] - Kw + 1
    return F.conv2d(x, w.flip(-2, -1), padding=(Kh - 1, Kw - 1))[..., :vh, :vw][..., ::stride[0], ::stride[1]]


def crandn(gen, *shape):
    return torch.complex(torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen))


def bin_contract_def(x, w):
    return torch.einsum("bpi,pio->bpo", x.to(torch.complex128), w.to(torch.complex128))


def bin_contract_grads_def(x, w, gy):
    """(gx, gw) in complex128, torch's convention (grad = dL/dRe + i dL/dIm)"""
    x, w, gy = (t.to(torch.complex128) for t in (x, w, gy))
    return torch.einsum("bpo,pio->bpi", gy, w.conj()), torch.einsum("bpi,bpo->pio", x.conj(), gy)


def matmul_def(x, w_freq):
    return torch.matmul(x.double(), torch.fft.ifft(w_freq.to(torch.complex128), dim=-1).real)


def separated_spectrum(shape, k, seed=SEED, complex_input=True):
    """A tensor whose k-th and (k+1)-th largest SQUARED magnitudes differ by more than a relative 1e-5 (asserted), so that
    torch.topk on torch.abs and the radix select on fl(re re + im im) keep the same set in the same order: distinct
    magnitudes on a geometric ladder with ratio 1 + 1e-3, in a random arrangement, each with a random phase."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    mags = 1.001 ** torch.arange(n, dtype=torch.float64)
    mags = (mags / mags.max())[torch.randperm(n, generator=g)]
    phase = torch.rand(n, generator=g, dtype=torch.float64) * (2 * np.pi) if complex_input else torch.zeros(n, dtype=torch.float64)
    z = torch.polar(mags, phase).to(torch.complex64).reshape(shape)
    sq = np.sort((z.real.double() ** 2 + z.imag.double() ** 2).numpy().reshape(-1))[::-1]
    assert np.all(sq[:-1] - sq[1:] > 1e-5 * sq[:-1]), "magnitudes are not separated"
    assert 1 <= k <= n
    return z


def spatial_with_separated_spectrum(shape, seed=SEED):
    """A REAL tensor is not what gives a separated spectrum (its spectrum is Hermitian: every magnitude twice), so the
    sparse-FFT cases transform a COMPLEX input: ifftn of separated_spectrum.  The separation of the spectrum that fftn
    gives back is asserted by the caller on the spectrum it actually ranks."""
    return torch.fft.ifftn(separated_spectrum(shape, 1, seed).to(torch.complex128)).to(torch.complex64)


def assert_separated(spectrum, k):
    """the k-th and (k+1)-th squared magnitudes of `spectrum` (and every neighbouring pair above them, which fixes the
    order) differ by more than a relative 1e-5"""
    sq = np.sort((spectrum.real.double() ** 2 + spectrum.imag.double() ** 2).cpu().numpy().reshape(-1))[::-1]
    top = sq[:k + 1] if k < sq.size else sq
    assert np.all(top[:-1] - top[1:] > 1e-5 * top[:-1]), "the spectrum's leading magnitudes are not separated"
