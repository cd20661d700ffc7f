"""Shared by the byte-spectral tests and tests/golden/make_golden_byte.py: the feature table of ByteSpectralEmbedding /
ByteSpectralEncoder restated in float64 from its definition (not from the reference's text), and the rule by which a
result is compared with it.  Nothing here imports the package under test or the reference.

    s[t] = float(id[t]) / 127.5 - 1,   S[f] = sum_t s[t] e^{-2 pi i f t / T},   k = min(W // 2, T // 2)
    column j of the row at (b, pos):   j <  k   |S[b, j]| bands[j]
                                  k <= j < 2k   Im(S[b, j - k] e^{i theta}) / |S[b, j - k]|     theta = 2 pi (f pos mod T) / T
                                 2k <= j < 3k   Re(S[b, j - 2k] e^{i theta}) / |S[b, j - 2k]|
                                 3k <= j        0
    cut at W columns; S == 0: sin 0, cos 1.  positions=False: the one row of pos = 0.

Comparison: the angle of a bin is conditioned like max_f |S| / |S|, and the reference's own phase columns are rounding
noise where |S| is tiny.  So a bin is COMPARABLE when its float64 |S| >= MIN_MAG; phase columns of other bins are left
out (their share is bounded by MAX_LEFT_OUT), magnitude columns are always compared.  Errors are normalised: magnitude
columns by max_f |S[b, f]| max|bands| of the row, phase columns by max_f |S[b, f]| / |S[b, f]|.
"""
import functools

import numpy as np

MIN_MAG = 0.1
MAX_LEFT_OUT = 0.01
TOL_FACTOR = 4.0        # a direct fp32 sum over T terms loses more than an FFT's log-depth sum, split accumulators or not

EMBEDDING_FIXTURES = ("Z01_byteemb_2x64x32", "Z02_byteemb_2x37x32", "Z03_byteemb_3x10x12", "Z04_byteemb_1x512x64")
ENCODER_FIXTURES = ("Z11_byteenc_2x100_M16", "Z12_byteenc_2x20_M16")
LM_FIXTURE = "Z21_bytelm_2x64x32"


def spectrum64(ids, k):
    """(B, k) complex128 bins of the rows.  Ids go through float32 first, as the reference's .float() does."""
    s = np.asarray(ids).astype(np.float32).astype(np.float64) / 127.5 - 1.0
    T = s.shape[1]
    n = (np.arange(k, dtype=np.int64)[:, None] * np.arange(T, dtype=np.int64)[None, :]) % T      # exact f t mod T
    return s @ np.exp(-2j * np.pi * n / T).T


def features64(ids, bands, W, positions=True):
    """The table: (B, T, W) float64, or (B, W) for positions=False."""
    ids = np.asarray(ids)
    B, T = ids.shape
    k = min(W // 2, T // 2)
    P = T if positions else 1
    out = np.zeros((B, P, W))
    if k:
        S = spectrum64(ids, k)
        mag = np.abs(S)
        n = (np.arange(P, dtype=np.int64)[:, None] * np.arange(k, dtype=np.int64)[None, :]) % T
        z = S[:, None, :] * np.exp(2j * np.pi * n / T)[None]
        u = np.where(mag[:, None, :] > 0, z / np.where(mag > 0, mag, 1.0)[:, None, :], 1.0 + 0.0j)
        full = np.concatenate([np.broadcast_to((mag * np.asarray(bands, np.float64)[:k])[:, None, :], (B, P, k)),
                               u.imag, u.real], axis=-1)
        w = min(W, 3 * k)
        out[..., :w] = full[..., :w]
    return out if positions else out[:, 0]


def compare(got, ids, bands, W, positions=True):
    """(largest normalised error, share of phase entries left out) of `got` against the table; asserts the padding to be
    exactly zero and the share to be at most MAX_LEFT_OUT."""
    ids = np.asarray(ids)
    B, T = ids.shape
    k = min(W // 2, T // 2)
    ref = features64(ids, bands, W, positions)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    if not positions:
        got, ref = got[:, None], ref[:, None]
    assert not got[..., 3 * k:].any()
    if k == 0:
        return 0.0, 0.0
    mag = np.abs(spectrum64(ids, k))                                     # (B, k)
    top = mag.max(axis=1)                                                # (B,)
    d = np.abs(got - ref)
    worst = float((d[..., :k] / (top * np.abs(np.asarray(bands, np.float64)[:k]).max())[:, None, None]).max())
    ok = mag >= MIN_MAG
    scale = np.where(ok, mag, 0.0) / top[:, None]                        # 1 / conditioning; 0 leaves the entry out
    total = left = 0
    for lo in (k, 2 * k):
        n = max(0, min(k, W - lo))
        if n:
            worst = max(worst, float((d[..., lo:lo + n] * scale[:, None, :n]).max()))
            total += B * got.shape[1] * n
            left += int((~ok[:, :n]).sum()) * got.shape[1]
    share = left / total if total else 0.0
    assert share <= MAX_LEFT_OUT, f"{share:.3%} of the phase entries belong to bins with |S| < {MIN_MAG}"
    return worst, share


@functools.lru_cache(None)
def r_ref():
    """The largest normalised error of the reference's own recorded features against the table, over all fixtures: the
    yardstick of the tolerance TOL_FACTOR * r_ref."""
    from conftest import load_golden
    r = 0.0
    for name in EMBEDDING_FIXTURES + ENCODER_FIXTURES + (LM_FIXTURE,):
        z = load_golden(name)
        pos = name not in ENCODER_FIXTURES
        e, share = compare(z["features"], z["ids"], z["bands"], int(z["width"]), positions=pos)
        assert share == 0.0, (name, share)                               # the fixtures leave out no bin
        r = max(r, e)
    return r


def loop64(ids, bands, W):
    """The reference's per-position procedure in float64 torch, differentiable in `bands` (a torch tensor): roll, FFT,
    abs, angle, sin, cos, cat, pad -- what grad_bands is checked against."""
    import torch
    ids = torch.as_tensor(np.asarray(ids))
    B, T = ids.shape
    k = min(W // 2, T // 2)
    s = ids.to(torch.float32).double() / 127.5 - 1.0
    rows = []
    for pos in range(T):
        spec = torch.fft.fft(torch.roll(s, -pos, dims=1), dim=1)[:, :k]
        f = torch.cat([spec.abs() * bands[:k], torch.sin(spec.angle()), torch.cos(spec.angle())], dim=-1)
        f = torch.nn.functional.pad(f, (0, W - 3 * k)) if 3 * k < W else f[:, :W]
        rows.append(f)
    return torch.stack(rows, dim=1)
