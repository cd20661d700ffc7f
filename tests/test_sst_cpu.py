"""The sparse spectral tensor without a GPU: exports, the argument checks of the smx_topk_* / smx_sparse_scatter entries,
the torch definition path against the numpy definition (bit for bit), parity with the reference's recorded results
(Q*.npz) under sst_common.check_membership, the axis walk of fftn / ifftn, and the reference's own unit tests restated.

Tolerance of the parity tests: on the CPU this package and the reference run the same torch ops on the same values
(scatter, torch.fft.ifftn, the activations, the pooling, matmul), so every compared result was measured at distance 0
from the golden (max-normalised).  The tests state TOL_CPU = 1e-6, about 8 fp32 ulps of the largest element: room for
another torch build's FFT, none for a wrong coefficient (the smallest kept coefficient moves a result by > 1e-3)."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import sst_common as sc
from conftest import ROOT, load_golden, rel_err

NAMES = ("SparseSpectralTensor", "MemoryManager", "sst", "zeros_sst", "randn_sst", "sparsify_topk", "sparse_scatter", "fftn",
         "ifftn", "spectral_normalize", "spectral_activation", "spectral_pool", "FrequencyMatMul")
ENTRIES = ("smx_topk_supported", "smx_topk_workspace_bytes", "smx_topk_select", "smx_topk_compact", "smx_sparse_scatter")
TOL_CPU = 1e-6


def pkg():
    import tensor_cuda_fft_amd
    return tensor_cuda_fft_amd


@pytest.fixture(scope="module")
def L():
    """the ctypes binding, with libsmx.so built first on a fresh checkout (as tests/test_abi.py does)"""
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


@pytest.fixture(autouse=True)
def fresh_manager():
    p = pkg()
    p.MemoryManager.clear_all()
    yield
    p.MemoryManager.clear_all()
    p.MemoryManager.set_limit(5000)


@pytest.fixture(scope="module")
def goldens():
    return {(shape, seed): load_golden(sc.golden_name(shape, seed)) for shape in sc.SHAPES for seed in sc.SEEDS}


def cpu_sst(x, sparsity=0.05):
    return pkg().sst(x, sparsity=sparsity, device="cpu")


# ---- names and signatures ---------------------------------------------------------------------------------------------------------
def test_names_are_exported_and_signatures_bound(L):
    p = pkg()
    for n in NAMES:
        assert n in p.__all__ and hasattr(p, n), n
    assert set(ENTRIES) <= set(L._SIGS)
    hdr = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "tensor.py:136-144" in hdr and "tensor.py:194-203" in hdr
    sig = inspect.signature(p.SparseSpectralTensor.__init__)
    assert list(sig.parameters)[1:] == ["data", "freq_coeffs", "indices", "shape", "sparsity", "device", "dtype",
                                        "use_cuda_backend"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["sparsity"], d["device"], d["dtype"], d["use_cuda_backend"]) == (0.05, "cuda", torch.float32, True)
    sig = inspect.signature(p.sparsify_topk)
    assert list(sig.parameters) == ["freq", "sparsity", "k", "max_workgroups"]
    assert sig.parameters["k"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(p.sparse_scatter).parameters["assume_ascending"].default is False
    for f in (p.sparsify_topk, p.sparse_scatter, p.fftn, p.ifftn):
        assert "ot differentiable" in f.__doc__
    for name in ("spectral_conv", "implicit_matmul", "ImplicitWeights", "spectral_backward"):
        assert not hasattr(p, name) and name in p.ops.__doc__


# ---- the C entries' argument checks -----------------------------------------------------------------------------------------------
def test_sst_entries_validate_without_touching_the_gpu(L):
    lib = L.lib()
    err = lambda: lib.smx_last_error().decode()
    assert [lib.smx_topk_supported(n) for n in (1, 2, 4096, 2 ** 31 - 1)] == [1] * 4
    assert [lib.smx_topk_supported(n) for n in (0, -1, 2 ** 31, 2 ** 40)] == [0] * 4
    nb = ctypes.c_size_t()
    assert lib.smx_topk_workspace_bytes(100, ctypes.byref(nb)) == 0 and nb.value % 256 == 0 and nb.value > 0
    small = nb.value
    assert lib.smx_topk_workspace_bytes(1 << 24, ctypes.byref(nb)) == 0 and nb.value > small
    assert lib.smx_topk_workspace_bytes(100, None) == -1 and "NULL" in err()
    assert lib.smx_topk_workspace_bytes(0, ctypes.byref(nb)) == -2 and "smx_topk_supported" in err()
    assert lib.smx_topk_workspace_bytes(2 ** 31, ctypes.byref(nb)) == -2
    lib.smx_topk_workspace_bytes(64, ctypes.byref(nb))
    zbuf = (ctypes.c_float * 160)()
    res = (ctypes.c_longlong * 4)()
    cbuf = (ctypes.c_float * 160)()
    ibuf = (ctypes.c_longlong * 80)()
    obuf = ctypes.create_string_buffer(64 * 8 + 32)
    ws = ctypes.create_string_buffer(nb.value + 512)
    z, r, c, i = (ctypes.addressof(b) for b in (zbuf, res, cbuf, ibuf))
    z = (z + 7) // 8 * 8
    o = (ctypes.addressof(obuf) + 15) // 16 * 16
    w = (ctypes.addressof(ws) + 255) // 256 * 256

    sel = lambda *a: lib.smx_topk_select(*a, None)
    assert sel(z, 0, 1, r, w, nb.value, 0) == -2 and "n=0" in err()
    assert sel(z, 2 ** 31, 1, r, w, nb.value, 0) == -2
    assert sel(None, 64, 3, r, w, nb.value, 0) == -1 and "non-NULL" in err()
    assert sel(z, 64, 3, None, w, nb.value, 0) == -1 and "non-NULL" in err()
    assert sel(z, 64, 0, r, w, nb.value, 0) == -1 and "k must be in 1..n" in err()
    assert sel(z, 64, 65, r, w, nb.value, 0) == -1 and "k=65 n=64" in err()
    assert sel(z + 4, 64, 3, r, w, nb.value, 0) == -1 and "8-byte aligned" in err()
    assert sel(z, 64, 3, r + 4, w, nb.value, 0) == -1 and "8-byte aligned" in err()
    assert sel(z, 64, 3, r, w, nb.value, -1) == -1 and "max_workgroups" in err()
    assert sel(z, 64, 3, r, None, 0, 0) == -4 and "workspace is NULL" in err()
    assert sel(z, 64, 3, r, w, nb.value - 1, 0) == -4 and "workspace has" in err()
    assert sel(z, 64, 3, r, w + 8, nb.value, 0) == -4 and "256-byte aligned" in err()

    com = lambda *a: lib.smx_topk_compact(*a, None)
    assert com(z, 0, r, c, i, 8, w, nb.value, 0) == -2
    assert com(z, 64, r, c, i, -1, w, nb.value, 0) == -1 and "capacity" in err()
    assert com(None, 64, r, c, i, 8, w, nb.value, 0) == -1 and "non-NULL" in err()
    assert com(z, 64, None, c, i, 8, w, nb.value, 0) == -1
    assert com(z, 64, r, None, i, 8, w, nb.value, 0) == -1
    assert com(z, 64, r, c, None, 8, w, nb.value, 0) == -1
    assert com(z, 64, r, c + 4, i, 8, w, nb.value, 0) == -1 and "8-byte aligned" in err()
    assert com(z, 64, r, c, i + 4, 8, w, nb.value, 0) == -1 and "8-byte aligned" in err()
    assert com(z, 64, r, c, i, 8, w, nb.value, -1) == -1 and "max_workgroups" in err()
    assert com(z, 64, r, c, i, 8, None, 0, 0) == -4 and "workspace is NULL" in err()
    assert com(z, 64, r, c, i, 8, w, nb.value - 1, 0) == -4 and "workspace has" in err()
    assert com(z, 64, r, c, i, 8, w + 8, nb.value, 0) == -4 and "256-byte aligned" in err()
    assert com(z, 64, r, None, None, 0, w, nb.value, 0) == 0                       # capacity 0: nothing to write, no launch

    sca = lambda *a: lib.smx_sparse_scatter(*a, None)
    assert sca(c, i, 3, o, 0, 0) == -2 and "n=0" in err()
    assert sca(c, i, 3, o, 2 ** 31, 0) == -2
    assert sca(c, i, -1, o, 64, 0) == -1 and "m must be in 0..n" in err()
    assert sca(c, i, 65, o, 64, 0) == -1 and "m=65 n=64" in err()
    assert sca(c, i, 3, None, 64, 0) == -1 and "non-NULL" in err()
    assert sca(None, i, 3, o, 64, 0) == -1 and "non-NULL" in err()
    assert sca(c, None, 3, o, 64, 0) == -1 and "non-NULL" in err()
    assert sca(c, i, 3, o + 8, 64, 0) == -1 and "16-byte aligned" in err()
    assert sca(c + 4, i, 3, o, 64, 0) == -1 and "8-byte aligned" in err()
    assert sca(c, i + 4, 3, o, 64, 0) == -1 and "8-byte aligned" in err()
    assert sca(c, i, 3, o, 64, -1) == -1 and "max_workgroups" in err()
    assert list(res) == [0, 0, 0, 0] and bytes(obuf) == bytes(len(obuf))          # nothing was written


# ---- the torch definition path equals the numpy definition ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [s for s in sc.SIZES if s <= 3 * sc.TILE + 5])
def test_torch_path_equals_the_numpy_definition_bit_for_bit(n):
    p = pkg()
    for ci, kind in enumerate(sc.CLASSES):
        z = sc.build(kind, n, 100 + ci)
        keys = sc.keys_np(z)
        t = torch.from_numpy(z)
        if kind == "offset_view":
            t = torch.cat([torch.zeros(1, dtype=torch.complex64), t])[1:]
        for k in sc.ks_for(n):
            want_c, want_i, _ = sc.sparsify_np(z, k, keys)
            got_c, got_i = p.sparsify_topk(t, k=k)
            assert got_i.dtype == torch.int64 and got_c.dtype == torch.complex64
            assert np.array_equal(got_i.numpy(), want_i), (kind, n, k)
            assert np.array_equal(got_c.numpy().view(np.uint32), want_c.view(np.uint32)), (kind, n, k)
            if kind in ("zeros", "mag5"):
                assert got_i.numel() == n
    z = sc.build("normal", n, 7)
    if n >= 3:
        z[n // 2] = complex(float("nan"), 1.0)
        got_c, got_i = p.sparsify_topk(torch.from_numpy(z), k=1)                   # a NaN ranks above everything
        assert got_i.tolist() == [n // 2]


def test_sparsify_topk_checks_its_arguments_and_follows_the_reference_k():
    p = pkg()
    z = torch.from_numpy(sc.build("normal", 1000, 1))
    for sparsity, k in ((0.05, 50), (0.0001, 1), (0.0499, 49), (1.0, 1000)):
        c, i = p.sparsify_topk(z.view(10, 100), sparsity)
        assert i.numel() == k and torch.equal(c, z[i])
    for bad in (z.real, z.to(torch.complex128), [1j]):
        with pytest.raises(TypeError):
            p.sparsify_topk(bad, 0.05)
    for kw in ({}, {"sparsity": 0.05, "k": 3}, {"k": 0}, {"k": 1001}, {"sparsity": 1.5}, {"k": 3, "max_workgroups": -1}):
        with pytest.raises(ValueError):
            p.sparsify_topk(z, **kw)
    with pytest.raises(ValueError):
        p.sparsify_topk(z[:0], 0.05)
    zg = z.clone().requires_grad_(True)                                             # the torch path carries the gather's gradient
    c, i = p.sparsify_topk(zg, k=10)
    c.abs().sum().backward()
    assert int((zg.grad != 0).sum()) == 10


def test_sparse_scatter_on_the_cpu_is_zeros_and_index_put():
    p = pkg()
    c = torch.from_numpy(sc.build("normal", 5, 3))
    i = torch.tensor([7, 0, 11, 3, 4])
    want = torch.zeros(12, dtype=torch.complex64)
    want[i] = c
    assert torch.equal(p.sparse_scatter(c, i, (3, 4)), want.view(3, 4))
    srt = torch.sort(i)
    assert torch.equal(p.sparse_scatter(c[srt.indices], srt.values, (12,), assume_ascending=True), want)
    assert torch.equal(p.sparse_scatter(c[:0], i[:0], (2, 2)), torch.zeros(2, 2, dtype=torch.complex64))
    for bad_c, bad_i in ((c.real, i), (c, i.int()), (c, i[:4]), (c.view(5, 1), i)):
        with pytest.raises(TypeError):
            p.sparse_scatter(bad_c, bad_i, (12,))
    with pytest.raises(ValueError):
        p.sparse_scatter(c, i, (12,), max_workgroups=-1)


# ---- the axis walk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5,), (4, 1, 6), (3, 4, 5, 2)])
def test_axis_walk_with_a_torch_transform_is_fftn(shape):
    from tensor_cuda_fft_amd import functional as F
    p = pkg()
    z = torch.randn(shape, dtype=torch.complex64, generator=torch.Generator().manual_seed(3))
    seen = []

    def fft1d(a):
        assert a.dim() == 3 and a.is_contiguous()
        seen.append(tuple(a.shape))
        return torch.fft.fft(a, dim=1)
    got = F._axis_walk(z, fft1d)
    n = z.numel()
    assert seen == [(int(np.prod(shape[:i])), s, int(np.prod(shape[i + 1:]))) for i, s in enumerate(shape) if s > 1]
    assert rel_err(got.numpy(), torch.fft.fftn(z).numpy()) <= 1e-6                  # fp32 transforms in another order
    inv = torch.conj_physical(F._axis_walk(z.conj().resolve_conj(), fft1d)) / n     # ifftn's composition
    assert rel_err(inv.numpy(), torch.fft.ifftn(z).numpy()) <= 1e-6
    assert torch.equal(p.fftn(z), torch.fft.fftn(z)) and torch.equal(p.ifftn(z), torch.fft.ifftn(z))   # CPU: torch.fft
    with pytest.raises(TypeError):
        p.fftn(z.real)


# ---- parity with the reference's recorded results ------------------------------------------------------------------------------------
def flat_of(indices, shape):
    return np.ravel_multi_index(tuple(np.asarray(indices, np.int64).T), shape)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_reference_goldens(goldens, shape):
    p = pkg()
    worst = 0.0
    for seed in sc.SEEDS:
        z = goldens[(shape, seed)]
        spectrum = torch.from_numpy(z["spectrum"])
        magnitude = torch.abs(spectrum).numpy().reshape(-1)
        assert rel_err(torch.fft.fftn(torch.from_numpy(z["x"]).to(torch.complex64)).numpy(), z["spectrum"]) <= TOL_CPU
        for sparsity in sc.SPARSITIES:
            q = sc.sp_tag(sparsity) + "."
            ref_flat = flat_of(z[q + "indices"], shape)
            # membership, order and coefficient bits, given the reference's spectrum
            c, i = p.sparsify_topk(spectrum, sparsity)
            sc.check_membership(i.numpy(), c.numpy(), ref_flat, z[q + "freq_coeffs"], magnitude)
            # the N-D indices of a tensor built from data
            mine = cpu_sst(torch.from_numpy(z["x"]), sparsity)
            assert mine.indices.dtype == torch.int64 and tuple(mine.indices.shape) == (len(mine.freq_coeffs), len(shape))
            assert np.array_equal(flat_of(mine.indices.numpy(), shape), mine._flat.numpy()) and mine.shape == shape
            # to_spatial and the ops, from the reference's own kept set
            t = p.SparseSpectralTensor(freq_coeffs=torch.from_numpy(z[q + "freq_coeffs"]),
                                       indices=torch.from_numpy(z[q + "indices"].astype(np.int64)), shape=shape,
                                       sparsity=sparsity, device="cpu")
            assert t._ascending and not t.use_cuda
            spatial = t.to_spatial()
            assert spatial.dtype == torch.float32 and tuple(spatial.shape) == shape
            errs = [rel_err(spatial.numpy(), z[q + "to_spatial"])]
            nrm = p.spectral_normalize(t)
            assert torch.equal(nrm.indices, t.indices)
            errs.append(rel_err(nrm.freq_coeffs.numpy(), z[q + "normalize"]))
            errs.append(check_op(p.spectral_activation(t, str(z["act_name"])), z, q + "act.", spatial))
            if len(shape) == 2:
                pooled = p.spectral_pool(t, 2, str(z["pool_mode"]))
                assert pooled.sparsity == float(z[q + "pool.sparsity"])
                errs.append(check_op(pooled, z, q + "pool.", spatial))
            print(f"{shape} seed {seed} sparsity {sparsity}: max-normalised distances {errs}")
            worst = max(worst, *errs)
    assert worst <= TOL_CPU


def check_op(result, z, prefix, spatial):
    """a re-sparsified result against the golden: the band rule on membership, coefficients within TOL_CPU"""
    spectrum = torch.fft.fftn(_op_input(z, prefix, spatial).to(torch.complex64))
    ref_flat = flat_of(z[prefix + "indices"], tuple(spectrum.shape))
    assert tuple(result.shape) == tuple(spectrum.shape)
    magnitude = torch.abs(spectrum).numpy().reshape(-1)
    thr = float(np.abs(z[prefix + "freq_coeffs"]).min())
    assert sc.band_count(magnitude, thr) <= sc.BAND_CAP
    mine = result._flat.numpy()
    differ = np.setxor1d(mine, ref_flat)
    assert (np.abs(magnitude[differ].astype(np.float64) - thr) <= sc.BAND * thr).all()
    _, a, b = np.intersect1d(mine, ref_flat, return_indices=True)
    return rel_err(result.freq_coeffs.numpy()[a], z[prefix + "freq_coeffs"][b])


def _op_input(z, prefix, spatial):
    if prefix.endswith("act."):
        return {"relu": torch.relu, "tanh": torch.tanh}[str(z["act_name"])](spatial)
    pool = torch.nn.functional.max_pool2d if str(z["pool_mode"]) == "max" else torch.nn.functional.avg_pool2d
    return pool(spatial[None, None], kernel_size=2).squeeze()


def test_block_streaming_matmul_matches_the_reference(goldens):
    p = pkg()
    z = goldens[((32, 32), 1)]
    q = sc.sp_tag(float(z["bsm.sparsity"])) + "."
    w = p.SparseSpectralTensor(freq_coeffs=torch.from_numpy(z[q + "freq_coeffs"]),
                               indices=torch.from_numpy(z[q + "indices"].astype(np.int64)), shape=(32, 32),
                               sparsity=float(z["bsm.sparsity"]), device="cpu")
    x = torch.from_numpy(z["bsm.x"])
    out = p.FrequencyMatMul.block_streaming_matmul(x, w, block_size=int(z["bsm.block_size"]))
    e = rel_err(out.numpy(), z["bsm.out"])
    print(f"block_streaming_matmul: max-normalised distance {e:.3g}")
    assert out.shape == (2, 3, 32) and e <= TOL_CPU
    whole = p.FrequencyMatMul.block_streaming_matmul(x, w, block_size=32)          # one block: the product itself
    assert rel_err(whole.numpy(), torch.matmul(x, w.to_spatial()).numpy()) <= TOL_CPU
    assert rel_err(out.numpy(), whole.numpy()) > 1e-2                               # ... which the blocked form is not
    assert "is not" in " ".join(p.FrequencyMatMul.block_streaming_matmul.__doc__.split())


def test_unordered_indices_take_the_torch_scatter():
    p = pkg()
    x = torch.randn(8, 8, generator=torch.Generator().manual_seed(5))
    t = cpu_sst(x, 0.2)
    perm = torch.randperm(len(t.freq_coeffs), generator=torch.Generator().manual_seed(6))
    u = p.SparseSpectralTensor(freq_coeffs=t.freq_coeffs[perm], indices=t.indices[perm], shape=(8, 8), device="cpu")
    assert t._ascending and not u._ascending
    assert torch.equal(u.to_spatial(), t.to_spatial())
    flat = p.SparseSpectralTensor(freq_coeffs=t.freq_coeffs, indices=t._flat, shape=(8, 8), device="cpu")   # 1-D indices
    assert torch.equal(flat.to_spatial(), t.to_spatial())
    with pytest.raises(ValueError):
        p.SparseSpectralTensor(freq_coeffs=t.freq_coeffs, indices=t.indices, device="cpu")
    with pytest.raises(ValueError):
        p.SparseSpectralTensor(device="cpu")


# ---- the reference's tests/unit/test_tensor.py, restated ---------------------------------------------------------------------------
def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_creation_and_reconstruction_bounds():
    x = randn(64, 64)
    t = cpu_sst(x, 0.05)
    assert t.shape == (64, 64) and t.compress_ratio() > 1.0 and len(t.freq_coeffs) < x.numel()
    assert t.device == "cpu" and t.dtype == torch.float32 and t.sparsity == 0.05 and t.use_cuda is False
    assert t.freq_coeffs.dtype == torch.complex64 and t.indices.dtype == torch.int64
    x = randn(32, 32, seed=1)
    r = cpu_sst(x, 0.1).to_spatial()
    err = torch.norm(r - x) / torch.norm(x)
    assert r.shape == x.shape and 0.01 < err < 0.95
    assert "SparseSpectralTensor(shape=(64, 64), sparsity=0.050, n_coeffs=" in repr(t)
    assert t.memory_mb() == (len(t.freq_coeffs) * 8 + t.indices.numel() * 8) / 1024 ** 2


def test_addition_scalar_multiplication_and_matmul():
    p = pkg()
    a, b = cpu_sst(randn(32, 32, seed=1)), cpu_sst(randn(32, 32, seed=2))
    c = a + b
    assert isinstance(c, p.SparseSpectralTensor) and c.shape == a.shape
    with pytest.raises(ValueError):
        a + cpu_sst(randn(16, 16))
    for d, s in ((a * 2.0, 2.0), (3.0 * a, 3.0), (a * 2, 2.0)):
        assert isinstance(d, p.SparseSpectralTensor) and d.shape == a.shape
        assert torch.equal(d.freq_coeffs, a.freq_coeffs * s) and torch.equal(d.indices, a.indices)   # nothing materialised
        assert rel_err(d.to_spatial().numpy(), (a.to_spatial() * s).numpy()) <= 1e-5
    h = a * b
    assert isinstance(h, p.SparseSpectralTensor) and h.shape == a.shape
    m = cpu_sst(randn(32, 64, seed=3)).matmul(cpu_sst(randn(64, 16, seed=4)))
    assert isinstance(m, p.SparseSpectralTensor) and m.shape == (32, 16)


def test_ratio_bounds_and_nd_tensors():
    assert 10.0 < cpu_sst(randn(100, 100), 0.05).compress_ratio() < 200.0
    x = randn(64, 64, seed=2)
    for sparsity in (0.01, 0.05, 0.1, 0.2):
        assert 0.5 / sparsity < cpu_sst(x, sparsity).compress_ratio() < 2.0 / sparsity
    for shape in ((64,), (32, 32), (16, 16, 16), (8, 8, 8, 8)):
        t = cpu_sst(randn(*shape, seed=3))
        assert t.shape == shape and t.to_spatial().shape == shape and t.indices.shape[1] == len(shape)


def test_zeros_and_randn_creation():
    p = pkg()
    z = p.zeros_sst((64, 64), device="cpu")
    r = p.randn_sst((64, 64), device="cpu")
    assert z.shape == (64, 64) and len(z.freq_coeffs) == 64 * 64                    # every coefficient ties at zero
    assert torch.equal(z.to_spatial(), torch.zeros(64, 64))
    assert r.shape == (64, 64) and not torch.allclose(r.to_spatial(), torch.zeros(64, 64))


def test_default_device_falls_back_to_the_cpu_with_the_reference_warning():
    p = pkg()
    if torch.cuda.is_available():
        assert p.sst(randn(8, 8)).use_cuda is True
        return
    with pytest.warns(UserWarning, match="CUDA not available, falling back to CPU"):
        t = p.sst(randn(8, 8))
    assert t.device == "cpu" and t.use_cuda is False
    with pytest.warns(UserWarning, match="CUDA not available"):
        assert p.zeros_sst((4, 4)).device == "cpu" and p.randn_sst((4, 4)).device == "cpu"


def test_memory_manager_limit_clear_all_and_stats():
    p = pkg()
    M = p.MemoryManager
    assert len(M._tensors) == 0
    a = cpu_sst(randn(64, 64))
    b = cpu_sst(randn(64, 64, seed=1))
    assert len(M._tensors) == 2 and M.total_memory_mb() == a.memory_mb() + b.memory_mb()
    stats = M.get_stats()
    assert {"n_tensors", "total_memory_mb", "limit_mb", "utilization"} <= set(stats) and stats["n_tensors"] == 2
    assert stats["limit_mb"] == 5000 and stats["utilization"] == stats["total_memory_mb"] / 5000
    assert ("cuda_allocated_mb" in stats) == torch.cuda.is_available()
    del b
    assert M.get_stats()["n_tensors"] == 1                                         # weak references: the live ones count
    M.clear_all()
    assert len(M._tensors) == 0 and a.to_spatial().shape == (64, 64)
    M.set_limit(1000)
    assert M._max_memory_mb == 1000
    with pytest.raises(ValueError):
        M.set_limit(0)
    M.set_limit(1)
    with pytest.raises(MemoryError, match="SST memory limit exceeded"):
        cpu_sst(randn(300, 300), 0.9)                                             # 81000 coefficients, 1.85 MB
