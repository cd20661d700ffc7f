"""Shared by the sparse-spectral-tensor tests (test_sst_cpu.py, test_sst_gpu.py), tests/golden/make_golden_sst.py and
tests/tools/sst_bench.py: the numpy definition of the top-k sparsify, the tile size of the native kernels, the input
builders and the rule by which a kept set is compared with the reference's.  Nothing here imports the package under test
or the reference."""
import numpy as np

TILE = 4096                     # complex elements per tile of the native passes and of the scatter (csrc/smx_sst.hip)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 1_048_579)
CLASSES = ("normal", "zeros", "mag5", "three_keys", "low_bits", "exponents", "one_inf", "offset_view")

# the goldens Q*.npz: every shape at every seed; each file holds every sparsity
SHAPES = ((64,), (32, 32), (16, 16, 16), (8, 8, 8, 8), (33, 7), (100, 100))
SPARSITIES = (0.01, 0.05, 0.2)
SEEDS = (1, 2)
BAND = 1e-5                     # membership may differ from the reference's only this close (relative) to its threshold
BAND_CAP = 4                    # ... and at most this many entries of a spectrum may lie that close (a condition)


def golden_name(shape, seed: int) -> str:
    return f"Q{SHAPES.index(tuple(shape)) * len(SEEDS) + SEEDS.index(seed) + 1:02d}_sst_" + "x".join(map(str, shape)) + f"_s{seed}"


def sp_tag(sparsity: float) -> str:
    return f"p{int(round(sparsity * 100)):02d}"


# ---- the definition -------------------------------------------------------------------------------------------------------------
def keys_np(z: np.ndarray) -> np.ndarray:
    """uint32 keys of a complex64 array: bits(fl(fl(re re) + fl(im im))) & 0x7fffffff, every step rounded to fp32"""
    z = np.ascontiguousarray(z, dtype=np.complex64).reshape(-1)
    ri = z.view(np.float32)
    re, im = ri[0::2], ri[1::2]
    with np.errstate(all="ignore"):
        rr = np.multiply(re, re, dtype=np.float32)
        ii = np.multiply(im, im, dtype=np.float32)
        s = np.add(rr, ii, dtype=np.float32)
    return s.view(np.uint32) & np.uint32(0x7fffffff)


def threshold_np(keys: np.ndarray, k: int) -> int:
    """the k-th largest key (a stable sort)"""
    return int(np.sort(keys, kind="stable")[keys.size - k])


def sparsify_np(z: np.ndarray, k: int, keys: np.ndarray = None, sorted_keys: np.ndarray = None):
    """(coeffs, flat indices int64 ascending, threshold key): everything with key >= the k-th largest key.  `keys` /
    `sorted_keys` (np.sort(keys, kind="stable")): computed once by a caller that sweeps k."""
    z = np.ascontiguousarray(z, dtype=np.complex64).reshape(-1)
    keys = keys_np(z) if keys is None else keys
    t = threshold_np(keys, k) if sorted_keys is None else int(sorted_keys[keys.size - k])
    idx = np.nonzero(keys >= np.uint32(t))[0].astype(np.int64)
    return z[idx], idx, t


def ks_for(n: int) -> tuple:
    return tuple(sorted({1, min(2, n), max(1, n // 20), max(1, n - 1), n}))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
_MAG5 = np.array([3 + 4j, 3 - 4j, -3 + 4j, -3 - 4j, 4 + 3j, 4 - 3j, -4 + 3j, -4 - 3j, 5, -5, 5j, -5j], dtype=np.complex64)


def build(kind: str, n: int, seed: int) -> np.ndarray:
    """n complex64 values of input class `kind`.  No non-zero square is below 2**-126.
    normal       seeded normal values (clipped away from the subnormal squares)
    zeros        all keys 0: m = n
    mag5         magnitude exactly 5 in its twelve Gaussian-integer forms: all keys 25, m = n
    three_keys   keys 9 (1 %), 4 (49 %: the threshold for k = n // 20, thousands of times across all tiles) and 1
    low_bits     re = 1 + j 2**-11, im = 0: squares exact in fp32, keys differ only in their low bits
    exponents    powers of two: keys differ only in the exponent
    one_inf      normal values and one inf
    offset_view  normal values; the GPU test views them one element into a buffer (8- but not 16-byte aligned)"""
    rng = np.random.default_rng(seed)
    if kind in ("normal", "one_inf", "offset_view"):
        ri = rng.standard_normal((n, 2)).astype(np.float32)
        ri[np.abs(ri) < 1e-15] = 1e-15
        if kind == "one_inf":
            ri[int(rng.integers(n)), int(rng.integers(2))] = np.inf
        return np.ascontiguousarray(ri).view(np.complex64).reshape(n)
    if kind == "zeros":
        return np.zeros(n, dtype=np.complex64)
    if kind == "mag5":
        return _MAG5[rng.integers(len(_MAG5), size=n)]
    if kind == "three_keys":
        u = rng.random(n)
        re = np.where(u < 0.01, 3.0, np.where(u < 0.5, 2.0, 1.0)).astype(np.float32)
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
        swap = rng.random(n) < 0.5                               # the value sits in re or in im
        out = np.zeros((n, 2), dtype=np.float32)
        out[~swap, 0] = (re * sign)[~swap]
        out[swap, 1] = (re * sign)[swap]
        return out.view(np.complex64).reshape(n)
    if kind == "low_bits":
        j = rng.integers(0, 2048, size=n).astype(np.float32)
        return (1.0 + j * np.float32(2.0 ** -11)).astype(np.float32).astype(np.complex64)
    if kind == "exponents":
        e = rng.integers(-60, 61, size=n)
        return np.ldexp(np.float32(1.0), e).astype(np.float32).astype(np.complex64)
    raise ValueError(kind)


def scatter_indices(n: int, m: int, seed: int) -> np.ndarray:
    """m strictly ascending int64 indices in [0, n): a seeded sample that, where m allows, holds the first and the last
    element of every tile (0, TILE - 1, TILE, 2 TILE - 1, ..., n - 1)"""
    if m == n:
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    edges = np.unique(np.clip(np.concatenate([np.arange(0, n, TILE), np.arange(TILE - 1, n, TILE), [n - 1]]), 0, n - 1))
    edges = edges[:m]
    pool = np.setdiff1d(rng.choice(n, size=min(n, m + edges.size), replace=False), edges)
    rest = rng.permutation(pool)[:m - edges.size]
    return np.sort(np.concatenate([edges, rest])).astype(np.int64)


# ---- comparison with the reference's kept set --------------------------------------------------------------------------------------
def band_count(ref_magnitude: np.ndarray, ref_threshold: float) -> int:
    """entries of a spectrum whose reference magnitude (torch.abs) lies within BAND (relative) of the reference threshold"""
    return int((np.abs(ref_magnitude.astype(np.float64) - ref_threshold) <= BAND * ref_threshold).sum())


def check_membership(idx, coeffs, ref_idx, ref_coeffs, ref_magnitude, tol=None):
    """The rule of the comparison with the reference: given the same spectrum, the kept set (flat indices `idx`, ascending,
    with `coeffs`) equals the reference's (`ref_idx`, `ref_coeffs`) in membership, order and coefficient bits, except
    for entries whose reference magnitude `ref_magnitude[i]` lies within BAND of the reference threshold (the smallest
    kept reference magnitude), of which there may be at most BAND_CAP in the spectrum.  `tol`: the coefficients come from
    another evaluation of the spectrum and agree within tol * max|ref_coeffs| instead of bit for bit.  Returns the number
    of entries whose membership differs."""
    idx, ref_idx = np.asarray(idx, np.int64), np.asarray(ref_idx, np.int64)
    coeffs, ref_coeffs = np.asarray(coeffs, np.complex64), np.asarray(ref_coeffs, np.complex64)
    assert (np.diff(idx) > 0).all() and (np.diff(ref_idx) > 0).all()
    thr = float(ref_magnitude[ref_idx].min())
    assert band_count(ref_magnitude, thr) <= BAND_CAP
    differ = np.setxor1d(idx, ref_idx)
    close = np.abs(ref_magnitude[differ].astype(np.float64) - thr) <= BAND * thr
    assert close.all(), (differ[~close], ref_magnitude[differ[~close]], thr)
    common, mine, theirs = np.intersect1d(idx, ref_idx, return_indices=True)
    if tol is None:
        assert np.array_equal(coeffs[mine].view(np.uint32), ref_coeffs[theirs].view(np.uint32))
    else:
        d = float(np.abs(coeffs[mine].astype(np.complex128) - ref_coeffs[theirs]).max() / np.abs(ref_coeffs).max())
        assert d <= tol, d
    return int(differ.size)
