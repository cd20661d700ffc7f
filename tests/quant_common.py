"""Shared by tests/test_quant_cpu.py, tests/test_quant_gpu.py and tests/golden/make_golden_quant.py: the cases of
fft_tensor/polar_quantization.py, zero_materialize.py and llamaizer.py, their float64 / complex128 definitions (the
yardsticks) and the rule by which integer codes are compared.

Codes are integers rounded from fp32 values, so a log2 or atan2 that differs in its last bit flips a code whose value before
rounding sits on a boundary.  The definitions therefore return the values BEFORE rounding, u and v, for a GIVEN range; a
code under test must equal the float64 code wherever that value lies further than BAND from a rounding boundary (a
half-integer for the polar codes, which round; an integer for log8, which truncates) and may differ by one inside it.
BAND is 1e-4 code units: the reference's own fp32 ops disagree with float64 only within 9.8e-6 of a boundary (recorded per
fixture as ref_worst_*), and the device's log2f / atan2f are allowed a few ulp where the host's are within one.  Every test
input must keep at most BAND_SHARE of its elements inside the band (band_share, computed from float64 alone)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SEED = 2472          # chosen so that every test input meets the band-share condition below (float64 alone decides)
BAND = 1e-4
BAND_SHARE = 2e-3

POLAR_CONFIGS = [(4, 8), (3, 5), (6, 10), (1, 1)]            # the reference's default, its two other configs, the smallest
POLAR_SHAPES = [(256, 128), (3, 1000), (1, 4099)]
LAYER_SEEDS = (0, 1)
LAYER_ARGS = (128, 128, 0.1)
# (B, Ci, Co, L, K, padding, stride)
CONV1D = [(2, 3, 5, 40, 7, 0, 1), (2, 3, 5, 40, 7, 3, 2), (2, 3, 5, 5, 7, 0, 1)]
CONV2D = (1, 2, 3, 16, 12, 3, 5, (1, 2), (2, 1))              # B, Ci, Co, H, W, Kh, Kw, padding, stride
CONV3D = (1, 2, 2, 4, 6, 8, 3)                                # B, Ci, Co, D, H, W, K
LINEAR = (2, 5, 16, 24)

MEMBERS = {
    "PolarQuantizer": ["__init__", "quantize", "dequantize"],
    "ConvolutionTheoremMatMul": ["frequency_linear", "frequency_conv1d", "frequency_conv2d", "frequency_conv3d",
                                 "frequency_linear_batched"],
    "WirtingerAutograd": ["forward", "backward"],
    "FrequencyLinearLayer": ["__init__", "forward", "compress_ratio"],
    "LogarithmicQuantizer": ["log8_encode", "log8_decode", "compress_sparse_freq", "decompress_sparse_freq"],
    "FFTConverter": ["convert_linear_to_frequency", "convert_model", "save_fft_model"],
    "": ["frequency_linear", "frequency_conv1d"],
}


def polar_name(shape):
    return "R%02d_polar_" % (11 + POLAR_SHAPES.index(tuple(shape))) + "x".join(str(v) for v in shape)


def crandn(gen, *shape):
    return torch.complex(torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen))


def polar_input(shape, seed=SEED):
    """the reference's own test input, randn * 0.5 in complex64: magnitudes span many octaves"""
    g = torch.Generator().manual_seed(seed + int(np.prod(shape)))
    return crandn(g, *shape) * 0.5


def log8_input(shape, seed=SEED):
    """fp32 values of both signs whose magnitudes span 1e-4 .. 1e2, inside and beyond the codec's range 2^-8 .. 2^8"""
    g = torch.Generator().manual_seed(seed + 7 * int(np.prod(shape)))
    return torch.randn(*shape, generator=g) * 10.0 ** (torch.rand(*shape, generator=g) * 5.0 - 3.0)


def special_polar(n=4099, seed=SEED):
    """polar_input with the special points in front: (+0, +0), the four axes (v an exact half-integer at (1, 0) and
    (+0, +0): in the band by construction), |z| = 1e-12 (clamped) and |z| = 1e15"""
    z = polar_input((n,), seed + 1)
    pts = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (6e-13, 8e-13), (-8e-13, 6e-13), (6e14, -8e14)]
    z[:len(pts)] = torch.tensor([complex(a, b) for a, b in pts], dtype=torch.complex64)
    return z


def constant_magnitude(n=1000):
    """every element has re^2 + im^2 == 25 exactly: all magnitude codes are 0"""
    pts = torch.tensor([3 + 4j, -3 + 4j, 3 - 4j, -3 - 4j, 4 + 3j, -4 + 3j, 4 - 3j, -4 - 3j, 5 + 0j, 0 + 5j],
                       dtype=torch.complex64)
    return pts[torch.arange(n) % len(pts)]


# ---- float64 definitions ------------------------------------------------------------------------------------------------------

def _np128(z):
    return z.detach().cpu().numpy().astype(np.complex128)


def polar_lg_def(z):
    zz = _np128(z)
    with np.errstate(divide="ignore"):
        return np.log2(np.maximum(np.hypot(zz.real, zz.imag), 1e-9))


def polar_range_def(z):
    lg = polar_lg_def(z)
    return float(lg.min()), float(lg.max())


def polar_uv_def(z, mag_bits, phase_bits, mag_range):
    """(u, v) in float64: the magnitude and phase values before rounding, for the given range"""
    zz = _np128(z)
    mag_min, mag_max = (float(v) for v in mag_range)
    u = (polar_lg_def(z) - mag_min) / (mag_max - mag_min + 1e-9) * (2 ** mag_bits - 1)
    v = (np.arctan2(zz.imag, zz.real) + np.pi) / (2 * np.pi) * (2 ** phase_bits - 1)
    return u, v


def polar_dequantize_def(mag_q, phase_q, mag_bits, phase_bits, mag_range):
    mq = mag_q.detach().cpu().numpy().astype(np.float64)
    pq = phase_q.detach().cpu().numpy().astype(np.float64)
    mag_min, mag_max = (float(v) for v in mag_range)
    mag = 2.0 ** (mq / (2 ** mag_bits - 1) * (mag_max - mag_min) + mag_min)
    ph = pq / (2 ** phase_bits - 1) * 2 * np.pi - np.pi
    return mag * (np.cos(ph) + 1j * np.sin(ph))


def log8_t_def(x):
    """(sign bit, t): t is the value before clamp and truncation"""
    xx = x.detach().cpu().numpy().astype(np.float64)
    return (xx >= 0).astype(np.int64), (np.log2(np.abs(xx) + 1e-8) + 8) / 16 * 127


def log8_decode_def(e):
    ee = e.detach().cpu().numpy().astype(np.int64)
    return (((ee >> 7) & 1) * 2.0 - 1.0) * 2.0 ** ((ee & 127) / 127.0 * 16 - 8)


# ---- the code comparison ------------------------------------------------------------------------------------------------------

def _boundary_distance(t, mode):
    t = np.asarray(t, np.float64)
    if mode == "round":
        return np.abs(t - (np.floor(t) + 0.5))
    return np.abs(t - np.rint(t))


def codes_def(t, top, mode):
    t = np.asarray(t, np.float64)
    c = np.rint(t) if mode == "round" else np.trunc(np.clip(t, 0, top))      # np.rint: half to even, as torch.round
    return np.clip(c, 0, top).astype(np.int64)


def band_share(t, mode):
    """the share of elements whose value before rounding lies within BAND of a rounding boundary"""
    finite = np.isfinite(t)
    return float(np.mean(_boundary_distance(np.where(finite, t, 0.25), mode) <= BAND))


def check_codes(codes, t, top, mode, band=BAND):
    """Asserts the rule of this module's docstring; returns (number of codes that differ from float64's, the largest
    distance from a boundary at which one differs)."""
    got = np.asarray(codes.detach().cpu().numpy() if isinstance(codes, torch.Tensor) else codes).astype(np.int64)
    want = codes_def(t, top, mode)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = got != want
    if not diff.any():
        return 0, 0.0
    dist = _boundary_distance(np.where(np.isfinite(t), t, 0.25), mode)
    worst = float(dist[diff].max())
    assert worst <= band, f"{int(diff.sum())} codes differ, one at {worst:.3g} code units from a rounding boundary"
    assert np.abs(got - want)[diff].max() <= 1, "a code inside the band differs by more than one"
    return int(diff.sum()), worst


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


# ---- transform-based ops, complex128 ------------------------------------------------------------------------------------------

def c128(t):
    return t.to(torch.complex128) if t.is_complex() else t.double()


def linear_def(x, w_freq, bias=None):
    y = torch.fft.ifft(torch.matmul(torch.fft.fft(c128(x), dim=-1), c128(w_freq)), dim=-1).real
    return y if bias is None else y + bias.double()


def conv_def(x, w_freq, stride, padding):
    """the reference's frequency_conv1d / 2d / 3d in complex128 (nd = x.dim() - 2), without its broadcast product"""
    nd = x.dim() - 2
    x, w = c128(x), c128(w_freq)
    stride = (stride,) * nd if isinstance(stride, int) else tuple(stride)
    padding = (padding,) * nd if isinstance(padding, int) else tuple(padding)
    K = w.shape[-1]
    if any(p > 0 for p in padding):
        x = F.pad(x, tuple(v for p in reversed(padding) for v in (p, p)))
    S = tuple(x.shape[2:])
    if nd == 1:
        w = F.pad(w, (0, S[0] - K)) if K < S[0] else w[..., :S[0]]
    else:
        w = F.pad(w, tuple(v for s, k in zip(reversed(S), reversed(w.shape[2:])) for v in (0, max(0, s - k))))
    dims = tuple(range(-nd, 0))
    letters = "xyz"[:nd]
    y = torch.fft.ifftn(torch.einsum(f"bi{letters},oi{letters}->bo{letters}", torch.fft.fftn(x, dim=dims), w), dim=dims).real
    if nd == 1 and padding[0] > 0:
        y = y[:, :, K // 2:y.shape[-1] - (K - K // 2 - 1)]
    return y[(slice(None), slice(None)) + tuple(slice(None, None, s) for s in stride)]


def conv1d_inputs(case, seed=SEED):
    B, Ci, Co, L, K, _, _ = case
    g = torch.Generator().manual_seed(seed + L + K)
    return torch.randn(B, Ci, L, generator=g), crandn(g, Co, Ci, K) / (Ci * K) ** 0.5


def conv2d_inputs(seed=SEED):
    B, Ci, Co, H, W, Kh, Kw, _, _ = CONV2D
    g = torch.Generator().manual_seed(seed + 2)
    return torch.randn(B, Ci, H, W, generator=g), crandn(g, Co, Ci, Kh, Kw) / (Ci * Kh * Kw) ** 0.5


def conv3d_inputs(seed=SEED):
    B, Ci, Co, D, H, W, K = CONV3D
    g = torch.Generator().manual_seed(seed + 3)
    return torch.randn(B, Ci, D, H, W, generator=g), crandn(g, Co, Ci, K, K, K) / (Ci * K ** 3) ** 0.5


def linear_inputs(B, N, D_in, D_out, seed=SEED, complex_x=False):
    g = torch.Generator().manual_seed(seed + 5 * D_in + D_out)
    x = crandn(g, B, N, D_in) if complex_x else torch.randn(B, N, D_in, generator=g)
    return x, crandn(g, D_in, D_out) / math.sqrt(D_in), torch.randn(D_out, generator=g)
