"""The four-step path (k_fs_a -> column kernel templated on the tile count L -> k_fs_b; n_fft = 256 L, more than 512
bins) on the GPU against float64 references:

* every tile count the plan accepts, through every column mode: filter forward / backward with a row scale (modes 0
  and 1, and the k_fs_gsc sum over the column blocks), spectrum only (mode 2), the rfft / irfft pair (mode 4,
  k_fs_synth) and the complex sequence FFT (mode 3).  These shapes have one tile per workgroup of k_fs_a / k_fs_b
  (fs_lc = 1) on purpose: they isolate the column kernels.
* the chunked tile walk of k_fs_a / k_fs_b (fs_lc > 1): prefetch of the next tile and of its twiddle, the LDS double
  buffer, the wrap at the chunk's end, the rotated start, the ragged last chunk, the non-XCD workgroup map and the
  second launch round past 512 workgroups -- also behind the three-launch causal convolution.
* the batch-grouped backward (option fs_bgroups) at every tile count it is instantiated for.

References: oracle.spectral_oracle.*_closed_ex (numpy FFT in float64), numpy.fft and torch.fft in float64.
Tolerances: TOL_ACT for y / grad_x / spectra, TOL_PARAM for parameter gradients.
"""
import contextlib

import numpy as np
import pytest
import torch

from conftest import TOL_ACT, TOL_PARAM, rel_err
from oracle import spectral_oracle as so
from test_next_rows_gpu import T, _pkg

pytestmark = pytest.mark.gpu

# fs_tiles_filter (csrc/smx_api.hip): 5 ... 32; 36 ... 64 step 4; 72 ... 128 step 8; 144 ... 256 step 16
TILE_COUNTS = [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
               36, 40, 44, 48, 52, 56, 60, 64, 72, 80, 88, 96, 104, 112, 120, 128,
               144, 160, 176, 192, 208, 224, 240, 256]
# the tile counts no GPU test had compared with a reference before this file
NEW_COUNTS = [6, 9, 10, 11, 13, 14, 18, 19, 20, 21, 22, 26, 27, 28, 29,
              40, 60, 72, 88, 96, 104, 112, 120, 160, 176, 192, 208, 224]
CFFT_COUNTS = [2, 4] + TILE_COUNTS          # smx_cfft_ex also runs below the 512-bin threshold of the filter plans


def full_shape(L):
    """(B, rows, D, n_fft, k): every row, every bin (Nyquist included)."""
    n = 256 * L
    return (2, n, 6, n, n // 2 + 1)


def padded_shape(L):
    """zero-padded rows, pruned bins, a ragged second channel tile"""
    n = 256 * L
    return (1, n - 100 - L, 34, n, (512 + n // 2) // 2 + 1)


# (B, rows, D, n_fft), L, nwg, fs_lc, chunks: every one walks more than one tile per workgroup of k_fs_a / k_fs_b
WALK = [
    ((80, 2048, 2, 2048), 8, 80, 2, 4),        # smallest wrap, rot alternates 0 / 1, full rows
    ((40, 7900, 2, 7936), 31, 40, 3, 11),      # ragged last chunk (one tile), rot % cnt, padded rows, odd L
    ((24, 9216, 4, 9216), 36, 24, 2, 18),      # two-level columns behind a chunked walk
    ((8, 61440, 2, 61440), 240, 8, 4, 60),     # longest transform, L2 = 16
    ((8, 7680, 66, 7680), 30, 24, 2, 15),      # three channel tiles, last ragged: the (lc >> 1)(dt & 1) term of rot
    ((3, 8000, 200, 8192), 32, 21, 2, 16),     # B = 3: non-XCD branch of wg_map, seven channel tiles, padded rows
    ((264, 1280, 2, 1280), 5, 264, 5, 1),      # one workgroup walks all L tiles (the production regime)
    ((520, 1280, 2, 1280), 5, 520, 5, 1),      # 520 > 512 workgroups: the second launch round, bid0 = 512
]
# the causal convolution's three launches on the same walk, fs_lc = 2: (B, rows, D, n_fft, options)
WALK_CONV = [(40, 2100, 2, 4096, {}), (80, 1024, 2, 2048, {"conv1": 0})]

SHAPES = [pytest.param(full_shape(L), id=f"L{L}-full") for L in TILE_COUNTS] \
    + [pytest.param(padded_shape(L), id=f"L{L}-padded") for L in TILE_COUNTS] \
    + [pytest.param(s + (s[3] // 2 + 1,), id="walk-%dx%dx%d" % s[:3]) for s, *_ in WALK]


def check(what, got, ref, tol):
    e = rel_err(got, ref)
    print(f"{what}: {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (what, e)


def c(t):
    return t.detach().cpu().numpy()


class Case:
    """Inputs of one shape and the float64 spectrum of x, built once for the tests of that shape; nobody writes to it."""

    def __init__(self, B, R, D, n, k):
        self.dims = (B, R, D, n, k)
        rng = np.random.default_rng([B, R, D, n, k])
        f32 = lambda a: a.astype(np.float32)
        self.x = f32(rng.standard_normal((B, R, D)))
        self.g = f32(rng.standard_normal((B, R, D)))
        self.wr = f32(1 + 0.5 * rng.standard_normal((D, k + 3)))      # three columns the transform does not keep
        self.wi = f32(0.5 * rng.standard_normal((D, k + 3)))
        self.sc = f32(0.5 + rng.random((B, D)))
        self.sr = f32(rng.standard_normal((B, k, D)))          # a spectrum / the gradient of one
        self.si = f32(rng.standard_normal((B, k, D)))
        self.X = np.fft.rfft(self.x.astype(np.float64), n=n, axis=1)[:, :k]


@pytest.fixture(scope="module", params=SHAPES)
def case(request):
    return Case(*request.param)


@pytest.fixture(autouse=True)
def options_are_left_as_found(gpu):
    from tensor_cuda_fft_amd import _lib
    before = _lib.effective_options()
    yield
    assert _lib.current_options() is None and _lib.effective_options() == before


def test_the_literal_tile_counts_are_what_the_plan_accepts(gpu):
    pkg, lib, fn = _pkg()
    assert len(TILE_COUNTS) == 52 and len(set(TILE_COUNTS)) == 52 and set(NEW_COUNTS) < set(TILE_COUNTS)
    assert len(NEW_COUNTS) == 28
    taken = []
    for L in range(1, 262):
        n = 256 * L
        p = lib.plan_ex(lib.smx_shape(1, n, 2, n // 2 + 1, n, n // 2 + 1))
        if p.path == lib.SMX_PATH_DECIMATED and p.bands == 0:
            taken.append(L)
    assert taken == TILE_COUNTS


@pytest.mark.parametrize("shape", [full_shape, padded_shape])
@pytest.mark.parametrize("L", TILE_COUNTS)
def test_tile_count_shapes_take_the_four_step_plan_one_tile_per_workgroup(gpu, L, shape):
    pkg, lib, fn = _pkg()
    B, R, D, n, k = shape(L)
    p = lib.plan_ex(lib.smx_shape(B, R, D, k, n, k))
    assert (p.path, p.bands, p.groups, p.L) == (lib.SMX_PATH_DECIMATED, 0, 1, L)
    assert p.nsplit == L                      # fs_lc = 1: this part isolates the column kernels


@pytest.mark.parametrize("shape,L,nwg,lc,chunks", WALK)
def test_chunked_walk_shapes_walk_several_tiles_per_workgroup(gpu, shape, L, nwg, lc, chunks):
    pkg, lib, fn = _pkg()
    B, R, D, n = shape
    p = lib.plan_ex(lib.smx_shape(B, R, D, n // 2 + 1, n, n // 2 + 1))
    assert (p.path, p.bands, p.groups) == (lib.SMX_PATH_DECIMATED, 0, 1)
    assert (p.L, p.nsplit, p.workgroups) == (L, chunks, nwg * chunks)
    assert lc > 1 and -(-L // chunks) == lc and -(-L // lc) == chunks


def test_filter_with_row_scale(gpu, case):
    """Column modes 0 and 1 (and the sum over the 9 / 33 / 65 / 129 column blocks behind d/d row_scale): y, grad_x,
    grad_W (factor included) and grad_row_scale against the closed form; unused weight columns exactly zero."""
    pkg, lib, fn = _pkg()
    B, R, D, n, k = case.dims
    xd, wrd, wid, scd = (T(a).to(gpu).requires_grad_(True) for a in (case.x, case.wr, case.wi, case.sc))
    y = fn.spectral_filter(xd, wrd, wid, None, n_fft=n, k=k, row_scale=scd)
    y.backward(T(case.g).to(gpu))
    torch.cuda.synchronize()
    y0, _ = so.forward_closed_ex(case.x, case.wr, case.wi, None, n, k)
    gx_ref, gwr_ref, gwi_ref, _ = so.backward_closed_ex(case.x, case.wr, case.wi, case.g * case.sc[:, None, :], n, k)
    check("y", c(y), y0 * case.sc[:, None, :], TOL_ACT)
    check("grad_x", c(xd.grad), gx_ref, TOL_ACT)
    check("grad_w_re", c(wrd.grad), gwr_ref, TOL_PARAM)
    check("grad_w_im", c(wid.grad), gwi_ref, TOL_PARAM)
    check("grad_row_scale", c(scd.grad), (case.g.astype(np.float64) * y0).sum(axis=1), TOL_PARAM)
    assert not c(wrd.grad)[:, k:].any() and not c(wid.grad)[:, k:].any()


def four_step_pair(lib, n):
    """At n_fft = 2048 the library sends rfft_bins / rfft / irfft to the eight-band kernels (k_full8, k_synth8) by
    default (tests/test_transform_pair_gpu.py covers that); option full8 = 0 sends them down the four-step path like
    every other length, which is what this file is about.  The filter and the sequence FFT need no such option."""
    return lib.options(full8=0) if n == 2048 else contextlib.nullcontext()


def test_spectrum_only(gpu, case):
    """Column mode 2: functional.rfft_bins against numpy's rfft."""
    pkg, lib, fn = _pkg()
    B, R, D, n, k = case.dims
    with four_step_pair(lib, n):
        X = fn.rfft_bins(T(case.x).to(gpu), k, n)
    check("rfft_bins", c(X), case.X, TOL_ACT)


def test_rfft_forward_and_backward(gpu, case):
    """functional.rfft: the spectrum (mode 2) and its gradient, a synthesis with weight one on every bin (mode 4)."""
    pkg, lib, fn = _pkg()
    B, R, D, n, k = case.dims
    xg = T(case.x).to(gpu).requires_grad_(True)
    with four_step_pair(lib, n):
        y = fn.rfft(xg, n, k)
        assert y.shape == (B, k, D) and y.dtype == torch.complex64
        y.backward(torch.complex(T(case.sr), T(case.si)).to(gpu))
    x64 = T(case.x).double().requires_grad_(True)
    y64 = torch.fft.rfft(x64, n=n, dim=1)[:, :k]
    y64.backward(torch.complex(T(case.sr).double(), T(case.si).double()))
    check("rfft", c(y), y64.detach().numpy(), TOL_ACT)
    check("rfft grad_x", c(xg.grad), x64.grad.numpy(), TOL_ACT)


def test_irfft_forward_and_backward(gpu, case):
    """functional.irfft: the Hermitian synthesis (mode 4, k_fs_synth) and its gradient, a scaled spectrum (mode 2)."""
    pkg, lib, fn = _pkg()
    B, R, D, n, k = case.dims
    s = torch.complex(T(case.sr), T(case.si))
    sg = s.to(gpu).requires_grad_(True)
    with four_step_pair(lib, n):
        y = fn.irfft(sg, n, R)
        assert y.shape == (B, R, D) and y.dtype == torch.float32
        y.backward(T(case.g).to(gpu))
    s64 = s.to(torch.complex128).requires_grad_(True)
    y64 = torch.fft.irfft(s64, n=n, dim=1)[:, :R]
    y64.backward(T(case.g).double())
    check("irfft", c(y), y64.detach().numpy(), TOL_ACT)
    # the imaginary parts of the DC / Nyquist rows do not reach y: their gradient is zero on both sides
    check("irfft grad_spec", torch.view_as_real(sg.grad.cpu()).numpy(), torch.view_as_real(s64.grad).numpy(), TOL_ACT)


def _seq_fft(gpu, B, N, Dc):
    pkg, lib, fn = _pkg()
    rng = np.random.default_rng([B, N, Dc])
    z = (rng.standard_normal((B, N, Dc)) + 1j * rng.standard_normal((B, N, Dc))).astype(np.complex64)
    out = fn.seq_fft_raw(T(z).to(gpu))
    assert fn._cfft_native[(B, N, 2 * Dc, N // 2 + 1, N, N // 2 + 1)]
    check("seq_fft", c(out), np.fft.fft(z.astype(np.complex128), axis=1), TOL_ACT)


@pytest.mark.parametrize("L", CFFT_COUNTS)
def test_complex_sequence_fft_at_every_tile_count(gpu, L):
    """Column mode 3 (smx_cfft_ex: full rows only), the 52 tile counts of the plan plus L = 2 and 4."""
    assert len(CFFT_COUNTS) == 54
    B, _, D, n, _ = full_shape(L)
    _seq_fft(gpu, B, n, D // 2)


@pytest.mark.parametrize("shape", [s for s, *_ in WALK], ids=lambda s: "%dx%dx%d" % s[:3])
def test_complex_sequence_fft_on_the_chunked_walk(gpu, shape):
    """k_fs_a with several tiles per workgroup feeding mode 3; the padded shapes as full rows of n_fft."""
    B, R, D, n = shape
    _seq_fft(gpu, B, n, D // 2)


@pytest.mark.parametrize("L", NEW_COUNTS)
def test_bias_gradient(gpu, L):
    """spectral_filter takes no bias together with a row scale: the bias gradient of the column kernels (mode 1) in a
    call of its own, at the tile counts no other test runs with a bias."""
    pkg, lib, fn = _pkg()
    B, R, D, n, k = full_shape(L)
    rng = np.random.default_rng([L, 1])
    x = rng.standard_normal((B, R, D)).astype(np.float32)
    g = rng.standard_normal((B, R, D)).astype(np.float32)
    wr = (1 + 0.5 * rng.standard_normal((D, k))).astype(np.float32)
    wi = (0.5 * rng.standard_normal((D, k))).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    xd, wrd, wid, bd = (T(a).to(gpu).requires_grad_(True) for a in (x, wr, wi, b))
    y = fn.spectral_filter(xd, wrd, wid, bd, n_fft=n, k=k)
    y.backward(T(g).to(gpu))
    torch.cuda.synchronize()
    y_ref, _ = so.forward_closed_ex(x, wr, wi, b, n, k)
    check("y", c(y), y_ref, TOL_ACT)
    check("grad_bias", c(bd.grad), g.astype(np.float64).sum(axis=(0, 1)), TOL_PARAM)


@pytest.mark.parametrize("B,R,D,n_fft,opts", WALK_CONV)
def test_rank_one_conv_on_the_chunked_walk(gpu, B, R, D, n_fft, opts):
    """smx_conv_forward / backward in three launches (k_fs_a, k_fs_conv, k_fs_b) with two tiles per workgroup, against
    float64 autograd of rfft -> * H -> irfft -> crop -> * s."""
    pkg, lib, fn = _pkg()
    rng = np.random.default_rng([B, R, D, n_fft])
    fb = n_fft // 2 + 1
    x = rng.standard_normal((B, R, D)).astype(np.float32)
    g = rng.standard_normal((B, R, D)).astype(np.float32)
    hr = rng.standard_normal(fb).astype(np.float32); hi = rng.standard_normal(fb).astype(np.float32)
    sc = (0.5 + rng.random((B, D))).astype(np.float32)
    L, nwg = n_fft // 256, B * -(-D // 32)
    lc = -(-L // min(max(512 // nwg, 1), L))
    assert lc == 2                                      # conv_plan's chunking (csrc/smx_api.hip)
    with lib.options(**opts):
        assert fn.conv_supported(B, R, D, n_fft)
        assert not lib.conv_io_supported(B, R, D, n_fft, lib.SMX_IO_BF16)   # three launches: no 2-byte rows there
        xd, hrd, hid, scd = (T(a).to(gpu).requires_grad_(True) for a in (x, hr, hi, sc))
        y = fn.rank_one_conv(xd, hrd, hid, scd, n_fft)
        y.backward(T(g).to(gpu))
        torch.cuda.synchronize()
    xt, hrt, hit, sct = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, hr, hi, sc))
    X = torch.fft.rfft(torch.nn.functional.pad(xt, (0, 0, 0, n_fft - R)), dim=1)
    yr = torch.fft.irfft(X * torch.complex(hrt, hit)[None, :, None], n=n_fft, dim=1)[:, :R] * sct[:, None, :]
    yr.backward(torch.tensor(g, dtype=torch.float64))
    check("y", c(y), yr.detach().numpy(), TOL_ACT)
    check("grad_x", c(xd.grad), xt.grad.numpy(), TOL_ACT)
    check("grad_scale", c(scd.grad), sct.grad.numpy(), TOL_PARAM)
    check("grad_h_re", c(hrd.grad), hrt.grad.numpy(), TOL_PARAM)
    check("grad_h_im", c(hid.grad), hit.grad.numpy(), TOL_PARAM)


@pytest.mark.parametrize("L", list(range(5, 17)))
def test_batch_grouped_backward(gpu, L):
    """k_fs_f_grouped<L> (option fs_bgroups = 8: the slab rows summed over batch groups inside the column launch) at
    every tile count it is instantiated for, against the closed form and against the default backward (another
    summation order, so not bitwise)."""
    pkg, lib, fn = _pkg()
    B, D, n = 16, 2, 256 * L
    k = n // 2 + 1
    rng = np.random.default_rng([L, 3])
    x = rng.standard_normal((B, n, D)).astype(np.float32)
    g = rng.standard_normal((B, n, D)).astype(np.float32)
    wr = (1 + 0.5 * rng.standard_normal((D, k))).astype(np.float32)
    wi = (0.5 * rng.standard_normal((D, k))).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)

    def run():
        xd, wrd, wid, bd = (T(a).to(gpu).requires_grad_(True) for a in (x, wr, wi, b))
        fn.spectral_filter(xd, wrd, wid, bd, n_fft=n, k=k).backward(T(g).to(gpu))
        torch.cuda.synchronize()
        return [c(t.grad) for t in (xd, wrd, wid, bd)]

    with lib.options(fs_bgroups=8):
        grouped = run()
    assert lib.current_options() is None
    default = run()
    refs = so.backward_closed_ex(x, wr, wi, g, n, k)
    for name, got, dflt, ref, tol in zip(("grad_x", "grad_w_re", "grad_w_im", "grad_bias"), grouped, default, refs,
                                         (TOL_ACT, TOL_PARAM, TOL_PARAM, TOL_PARAM)):
        check(name, got, ref, tol)
        check(name + " vs default", got, dflt, TOL_PARAM)
