"""The sparse spectral tensor on the GPU: the native top-k sparsify (csrc/smx_sst.hip) against the numpy definition on the
same input bits -- exact equality of m, indices and coefficients over every size, input class, k and workgroup count the
kernels treat differently --, its reproducibility, the native scatter against zeros + index_put_ bit for bit (eager and
captured in a graph), and sst(x) / to_spatial() / block_streaming_matmul against the reference's recorded results.

Tolerance against the goldens: the device path transforms with the native fp32 sequence transform axis by axis, the
reference with torch.fft on the CPU; both are fp32 transforms of at most 4096 points, whose results differ by a few
ulps of the largest element times log2(points).  The tests hold them to TOL_ACT = 1e-5 (max-normalised), the project's
stated tolerance for fp32 activations (conftest.py); the measured distances are printed and recorded in DESIGN.md 7n."""
import numpy as np
import pytest
import torch

import sst_common as sc
from conftest import TOL_ACT, load_golden, rel_err

pytestmark = pytest.mark.gpu
TILE = sc.TILE
GPU_SHAPES = ((32, 32), (16, 16, 16), (8, 8, 8, 8), (64,), (33, 7), (100, 100))
N_PAST_1024 = 1025 * TILE + 5   # local to this file: the CPU tests share sst_common.SIZES and stay as light as they are


def pkg():
    import tensor_cuda_fft_amd
    return tensor_cuda_fft_amd


def on_device(kind, z, gpu):
    """the input on the device; class offset_view one element into a buffer: 8- but not 16-byte aligned"""
    t = torch.from_numpy(z)
    if kind != "offset_view":
        return t.to(gpu)
    buf = torch.zeros(z.size + 1, dtype=torch.complex64, device=gpu)
    buf[1:].copy_(t)
    assert buf[1:].data_ptr() % 16 == 8
    return buf[1:]


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy()).view(np.uint32)


# ---- sparsify_topk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.SIZES)
def test_native_sparsify_equals_the_definition_exactly(gpu, n):
    """every input class at this size; every k (two per class at the largest size, all five over the classes); the
    workgroup caps 0, 1, 2 in rotation, so each meets every size"""
    p = pkg()
    seen_mw = set()
    for ci, kind in enumerate(sc.CLASSES):
        z = sc.build(kind, n, 100 + ci)
        keys = sc.keys_np(z)
        srt = np.sort(keys, kind="stable")
        dev = on_device(kind, z, gpu)
        ks = sc.ks_for(n)
        if n > 100_000:
            ks = tuple(ks[(ci + j) % len(ks)] for j in (0, 2))
        for ki, k in enumerate(ks):
            mw = (ci + ki) % 3
            seen_mw.add(mw)
            want_c, want_i, _ = sc.sparsify_np(z, k, keys, srt)
            got_c, got_i = p.sparsify_topk(dev, k=k, max_workgroups=mw)
            assert got_c.dtype == torch.complex64 and got_i.dtype == torch.int64 and got_c.device == dev.device
            assert got_i.numel() == want_i.size, (kind, n, k, mw, got_i.numel(), want_i.size)
            assert np.array_equal(got_i.cpu().numpy(), want_i), (kind, n, k, mw)
            assert np.array_equal(bits(got_c), want_c.view(np.uint32)), (kind, n, k, mw)
            if kind in ("zeros", "mag5"):
                assert got_i.numel() == n
    assert seen_mw == {0, 1, 2} or n == 1


@pytest.mark.parametrize("kind", ["normal", "three_keys", "offset_view"])
def test_native_sparsify_past_1024_tiles(gpu, kind):
    """N_PAST_1024 elements are 1026 tiles (1027 for offset_view, which starts one element into its first tile): each of
    k_topk_scan's 1024 threads owns two tiles and the last 511 none; under the default caps (max_workgroups = 0) the
    histogram pass walks three tiles per workgroup and the count / write passes two."""
    p = pkg()
    n = N_PAST_1024
    z = sc.build(kind, n, 300 + sc.CLASSES.index(kind))
    keys = sc.keys_np(z)
    srt = np.sort(keys, kind="stable")
    dev = on_device(kind, z, gpu)
    for k in (n // 20, n - 1):
        want_c, want_i, _ = sc.sparsify_np(z, k, keys, srt)
        got_c, got_i = p.sparsify_topk(dev, k=k, max_workgroups=0)
        assert got_i.numel() == want_i.size, (kind, k, got_i.numel(), want_i.size)
        assert np.array_equal(got_i.cpu().numpy(), want_i), (kind, k)
        assert np.array_equal(bits(got_c), want_c.view(np.uint32)), (kind, k)
        if kind == "three_keys" and k == n // 20:                   # ... and back: the scatter over 1026 tiles
            assert got_i.numel() > n // 3                           # the tie at the threshold is kept whole
            want = torch.zeros(n, dtype=torch.complex64, device=gpu)
            want.index_put_((got_i,), got_c)
            back = p.sparse_scatter(got_c, got_i, (n,), assume_ascending=True)
            assert torch.equal(torch.view_as_real(back).view(torch.int32), torch.view_as_real(want).view(torch.int32))


def test_native_sparsify_is_reproducible_and_takes_sparsity_and_shapes(gpu):
    p = pkg()
    n = 3 * TILE + 5
    z = sc.build("three_keys", n, 9)
    dev = torch.from_numpy(z).to(gpu)
    first = p.sparsify_topk(dev, k=n // 20)
    second = p.sparsify_topk(dev, k=n // 20)
    assert torch.equal(first[1], second[1]) and np.array_equal(bits(first[0]), bits(second[0]))
    assert first[1].numel() > 1000                                  # the tie at the threshold is kept whole
    x = sc.build("normal", 96 * 128, 10)
    want_c, want_i, _ = sc.sparsify_np(x, max(1, int(x.size * 0.05)))
    got_c, got_i = p.sparsify_topk(torch.from_numpy(x).to(gpu).view(96, 128), 0.05)
    assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(bits(got_c), want_c.view(np.uint32))
    strided = torch.from_numpy(np.stack([x, x], axis=1)).to(gpu)[:, 0]          # made contiguous, then native
    got_c, got_i = p.sparsify_topk(strided, 0.05)
    assert np.array_equal(got_i.cpu().numpy(), want_i)


def test_native_sparsify_with_a_nan_stays_in_range(gpu):
    p = pkg()
    n = 257
    z = sc.build("normal", n, 11)
    z[100] = complex(float("nan"), 0.5)
    dev = torch.from_numpy(z).to(gpu)
    for k in (1, 13, n):
        c, i = p.sparsify_topk(dev, k=k)
        i = i.cpu().numpy()
        assert i.size >= k and (np.diff(i) > 0).all() and i[0] >= 0 and i[-1] < n
        assert 100 in i                                             # a NaN key ranks above everything
        assert np.array_equal(bits(c), z[i].view(np.uint32))
    assert p.sparsify_topk(dev, k=1)[1].tolist() == [100]


def test_native_threshold_key_is_the_definitions(gpu):
    """smx_topk_select's result (m, T) against numpy's: a key that is fused on the device (fl(re re + fl(im im))) is one
    ulp off for about a quarter of the elements and shows here at once, where membership alone would rarely move"""
    from tensor_cuda_fft_amd import functional as F
    n = 3 * TILE + 5
    for ci, kind in enumerate(("normal", "offset_view")):
        z = sc.build(kind, n, 200 + ci)
        keys = sc.keys_np(z)
        srt = np.sort(keys, kind="stable")
        dev = on_device(kind, z, gpu)
        ws = torch.empty(F._topk_ws_bytes(n), dtype=torch.uint8, device=gpu)
        for k in range(1, 400, 7):
            res = torch.empty(2, dtype=torch.int64, device=gpu)
            F._call(gpu, "smx_topk_select", dev.data_ptr(), n, k, res.data_ptr(), ws.data_ptr(), ws.numel(), k % 3, F._stream(gpu))
            t = int(srt[n - k])
            assert res.tolist() == [int((keys >= t).sum()), t], (kind, k)


# ---- sparse_scatter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.SIZES)
def test_native_scatter_equals_zeros_and_index_put(gpu, n):
    p = pkg()
    for mi, m in enumerate(sorted({0, 1, n // 20, n})):
        idx = sc.scatter_indices(n, m, 50 + mi)
        assert idx.size == m and (m in (0, n) or m < 8 or {0, n - 1} <= set(idx.tolist()))
        c = torch.from_numpy(sc.build("normal", m, 60 + mi)).to(gpu) if m else torch.empty(0, dtype=torch.complex64, device=gpu)
        i = torch.from_numpy(idx).to(gpu)
        want = torch.zeros(n, dtype=torch.complex64, device=gpu)
        want.index_put_((i,), c)
        for mw in (0, 1, 2) if n > TILE else ((mi % 3),):
            got = p.sparse_scatter(c, i, (n,), assume_ascending=True, max_workgroups=mw)
            assert got.shape == (n,) and got.dtype == torch.complex64
            assert torch.equal(torch.view_as_real(got).view(torch.int32), torch.view_as_real(want).view(torch.int32)), (n, m, mw)
    if n >= 64:                                                     # unordered indices: the torch route, same answer
        perm = torch.randperm(i.numel(), generator=torch.Generator().manual_seed(1)).to(gpu)
        assert torch.equal(p.sparse_scatter(c[perm], i[perm], (n,)), want)


def test_native_scatter_is_captured_in_a_graph(gpu):
    """no host synchronisation in the op: one captured call, replayed over new coefficients"""
    p = pkg()
    n, m = 2 * TILE + 50, 700
    i = torch.from_numpy(sc.scatter_indices(n, m, 3)).to(gpu)
    first = torch.from_numpy(sc.build("normal", m, 4)).to(gpu)
    second = torch.from_numpy(sc.build("normal", m, 5)).to(gpu)
    buf = first.clone()
    eager = p.sparse_scatter(first, i, (n,), assume_ascending=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p.sparse_scatter(buf, i, (n,), assume_ascending=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = p.sparse_scatter(buf, i, (n,), assume_ascending=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, p.sparse_scatter(second, i, (n,), assume_ascending=True)) and not torch.equal(out, eager)


# ---- the tensor on the device against the reference's recorded results -----------------------------------------------------------
def flat_of(indices, shape):
    return np.ravel_multi_index(tuple(np.asarray(indices, np.int64).T), shape)


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sst_on_the_device_matches_the_reference(gpu, shape):
    p = pkg()
    p.MemoryManager.clear_all()
    worst = 0.0
    for seed in sc.SEEDS:
        z = load_golden(sc.golden_name(shape, seed))
        magnitude = torch.abs(torch.from_numpy(z["spectrum"])).numpy().reshape(-1)
        spec_err = rel_err(p.fftn(torch.from_numpy(z["x"]).to(gpu).to(torch.complex64)).cpu().numpy(), z["spectrum"])
        for sparsity in sc.SPARSITIES:
            q = sc.sp_tag(sparsity) + "."
            ref_flat = flat_of(z[q + "indices"], shape)
            t = p.sst(torch.from_numpy(z["x"]).to(gpu), sparsity=sparsity)
            assert t.use_cuda and t.shape == shape and t.freq_coeffs.is_cuda and t.indices.is_cuda
            assert tuple(t.indices.shape) == (len(t.freq_coeffs), len(shape)) and t.indices.dtype == torch.int64
            assert np.array_equal(flat_of(t.indices.cpu().numpy(), shape), t._flat.cpu().numpy())
            differ = sc.check_membership(t._flat.cpu().numpy(), t.freq_coeffs.cpu().numpy(), ref_flat, z[q + "freq_coeffs"],
                                         magnitude, tol=TOL_ACT)
            # to_spatial: from the reference's own kept set, and from the tensor's where the two sets are the same
            r = p.SparseSpectralTensor(freq_coeffs=torch.from_numpy(z[q + "freq_coeffs"]),
                                       indices=torch.from_numpy(z[q + "indices"].astype(np.int64)), shape=shape,
                                       sparsity=sparsity)
            assert r.use_cuda and r._ascending
            spatial = r.to_spatial()
            assert spatial.is_cuda and spatial.dtype == torch.float32 and tuple(spatial.shape) == shape
            errs = [spec_err, rel_err(spatial.cpu().numpy(), z[q + "to_spatial"])]
            if differ == 0:
                errs.append(rel_err(t.to_spatial().cpu().numpy(), z[q + "to_spatial"]))
            print(f"{shape} seed {seed} sparsity {sparsity}: membership differs at {differ}, max-normalised distances "
                  f"(spectrum, to_spatial of the golden set, to_spatial of sst(x)) {errs}")
            worst = max(worst, *errs)
    assert worst <= TOL_ACT
    p.MemoryManager.clear_all()


@pytest.mark.parametrize("shape", [(512, 3), (3, 512), (100, 100), (48, 20, 6), (1, 7, 1), (257, 256, 12)],
                         ids=lambda s: "x".join(map(str, s)))
def test_fftn_and_ifftn_on_the_device_against_float64(gpu, shape):
    """The axis-by-axis transforms against numpy's on the complex128 copy of the same input, max-normalised, and their
    round trip.  (3, 512): the last axis as a one-channel native transform; (257, 256, 12): the last axis is a batch of
    65792 rows of 12 points -- more than one grid axis holds -- and the first a prime length; (1, 7, 1): axes of length
    1 are skipped."""
    p = pkg()
    rng = np.random.default_rng(sum(shape))
    z = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    dev = torch.from_numpy(z).to(gpu)
    z64 = z.astype(np.complex128)
    fwd, inv = p.fftn(dev), p.ifftn(dev)
    assert fwd.is_cuda and fwd.dtype == torch.complex64 and tuple(fwd.shape) == shape and tuple(inv.shape) == shape
    errs = {"fftn": rel_err(fwd.cpu().numpy(), np.fft.fftn(z64)), "ifftn": rel_err(inv.cpu().numpy(), np.fft.ifftn(z64)),
            "ifftn(fftn(z))": rel_err(p.ifftn(fwd).cpu().numpy(), z64)}
    print(f"{shape}: max-normalised distances to float64 {errs}; bound {TOL_ACT:.0e}")
    assert max(errs.values()) <= TOL_ACT, errs
    assert torch.equal(dev, torch.from_numpy(z).to(gpu))           # the input is left as it was


def test_block_streaming_matmul_on_the_device_matches_the_reference(gpu):
    p = pkg()
    z = load_golden(sc.golden_name((32, 32), 1))
    q = sc.sp_tag(float(z["bsm.sparsity"])) + "."
    w = p.SparseSpectralTensor(freq_coeffs=torch.from_numpy(z[q + "freq_coeffs"]),
                               indices=torch.from_numpy(z[q + "indices"].astype(np.int64)), shape=(32, 32),
                               sparsity=float(z["bsm.sparsity"]))
    out = p.FrequencyMatMul.block_streaming_matmul(torch.from_numpy(z["bsm.x"]).to(gpu), w, block_size=int(z["bsm.block_size"]))
    e = rel_err(out.cpu().numpy(), z["bsm.out"])
    print(f"block_streaming_matmul on the device: max-normalised distance {e:.3g}")
    assert out.is_cuda and e <= TOL_ACT
    p.MemoryManager.clear_all()
