"""The native transform along the contiguous last axis (csrc/smx_rowfft.hip, include/smx_rowfft.h) on the GPU.

Yardstick: np.fft.fft on the complex128 copy of the same input, max-normalised (conftest.rel_err), bound TOL_ACT = 1e-5 --
the project's stated tolerance for fp32 activations; the measured distances are printed and the largest is quoted in
DESIGN.md 7r.  Everything that the header promises bit for bit (row independence, the walk, in place, capture, real input
against complex input with a zero imaginary part) is compared on the bits."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from conftest import TOL_ACT, rel_err

pytestmark = pytest.mark.gpu
LENGTHS = tuple(2 ** i for i in range(1, 13))


def pkg():
    import tensor_cuda_fft_amd
    return tensor_cuda_fft_amd


def fnmod():
    from tensor_cuda_fft_amd import functional
    return functional


def rand_c64(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def bits(t):
    t = t.detach()
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def definition(x, conj_in, conj_out, real_out, scale):
    """include/smx_rowfft.h in float64"""
    a = x.astype(np.complex128)
    if conj_in:
        a = a.conj()
    y = np.fft.fft(a, axis=-1) * scale
    if conj_out:
        y = y.conj()
    return y.real if real_out else y


@pytest.mark.parametrize("n", LENGTHS)
def test_every_length_against_float64(gpu, n):
    """rows 1, 3 and 67: a lone row, and odd counts that end inside a workgroup's tile of 4096 / n rows (67 rows of 128
    points and more are several tiles, the last one partly filled)"""
    p = pkg()
    for rows in (1, 3, 67):
        z = rand_c64((rows, n), 1000 * n + rows)
        got = p.row_fft_raw(torch.from_numpy(z).to(gpu))
        assert got.dtype == torch.complex64 and tuple(got.shape) == (rows, n)
        e = rel_err(got.cpu().numpy(), np.fft.fft(z.astype(np.complex128), axis=-1))
        print(f"n={n} rows={rows}: max-normalised distance to float64 {e:.2e}; bound {TOL_ACT:.0e}")
        assert e <= TOL_ACT, (n, rows, e)


@pytest.mark.parametrize("n", [64, 1024])
def test_every_flag_combination(gpu, n):
    """conj_in x conj_out x real_out x (real | complex input), scale 1 and 1 / n: all sixteen flag words of the C entry
    (REAL_IN is implied by a float32 input).  A float32 input gives the bits of the complex input (x, +0)."""
    p = pkg()
    rows = 5
    z = rand_c64((rows, n), n)
    worst = 0.0
    for real_in, conj_in, conj_out, real_out in itertools.product((False, True), repeat=4):
        x = z.real.copy() if real_in else z
        dev = torch.from_numpy(x).to(gpu)
        for scale in (1.0, 1.0 / n):
            got = p.row_fft_raw(dev, conj_in=conj_in, conj_out=conj_out, real_out=real_out, scale=scale)
            assert got.dtype == (torch.float32 if real_out else torch.complex64) and tuple(got.shape) == (rows, n)
            e = rel_err(got.cpu().numpy(), definition(x, conj_in, conj_out, real_out, scale))
            worst = max(worst, e)
            assert e <= TOL_ACT, (real_in, conj_in, conj_out, real_out, scale, e)
            if real_in:
                as_complex = torch.from_numpy(x.astype(np.complex64)).to(gpu)
                want = p.row_fft_raw(as_complex, conj_in=conj_in, conj_out=conj_out, real_out=real_out, scale=scale)
                assert same_bits(got, want), (conj_in, conj_out, real_out, scale)
    print(f"n={n}: largest max-normalised distance over the 32 cases {worst:.2e}; bound {TOL_ACT:.0e}")


@pytest.mark.parametrize("n", [8, 256, 4096])
def test_a_row_does_not_depend_on_its_neighbours_or_the_grid(gpu, n):
    p = pkg()
    dev = torch.from_numpy(rand_c64((5, n), n + 1)).to(gpu)
    whole = p.row_fft_raw(dev)
    assert same_bits(whole, p.row_fft_raw(dev))                       # two identical calls
    assert same_bits(whole, p.row_fft_raw(dev, max_workgroups=1))
    for r in range(5):
        alone = p.row_fft_raw(dev[r].clone(), max_workgroups=1)
        assert same_bits(alone, whole[r]), (n, r)


def test_the_walk_past_a_16_bit_grid_axis(gpu):
    """70001 rows of 16 points -- more rows than one 16-bit grid axis holds -- against the same data in two halves.  The
    launcher never asks for more than 1024 workgroups: a workgroup owns 256 such rows at a time, so these are 274 row
    groups, walked under a lowered cap; 262401 rows are 1026 groups, one more round than the default grid holds."""
    p = pkg()
    n = 16
    for rows, caps in ((70001, (0, 3)), (1025 * 256 + 1, (0,))):
        dev = torch.from_numpy(rand_c64((rows, n), 7)).to(gpu)
        h = rows // 2 - (rows // 2) % 2 + 1                            # odd: the halves' row groups hold other rows
        halves = torch.cat((p.row_fft_raw(dev[:h]), p.row_fft_raw(dev[h:])))
        for cap in caps:
            assert same_bits(p.row_fft_raw(dev, max_workgroups=cap), halves), (rows, cap)
        e = rel_err(halves[-3:].cpu().numpy(), np.fft.fft(dev[-3:].cpu().numpy().astype(np.complex128), axis=-1))
        assert e <= TOL_ACT, e


def test_in_place(gpu):
    p = pkg()
    z = torch.from_numpy(rand_c64((3, 4096), 11)).to(gpu)
    want = p.row_fft_raw(z)
    assert p.row_fft_raw(z, out=z) is z and same_bits(z, want)
    x = torch.from_numpy(rand_c64((67, 128), 12).real.copy()).to(gpu)
    want = p.row_fft_raw(x, conj_out=True, real_out=True, scale=1.0 / 128)
    assert want.dtype == torch.float32
    assert p.row_fft_raw(x, conj_out=True, real_out=True, scale=1.0 / 128, out=x) is x and same_bits(x, want)
    with pytest.raises(ValueError):
        p.row_fft_raw(z, out=x)


def test_capture_and_replay(gpu):
    p = pkg()
    a, b = (torch.from_numpy(rand_c64((67, 256), s)).to(gpu) for s in (21, 22))
    eager = [p.row_fft_raw(t, conj_in=True, scale=0.5) for t in (a, b)]
    x, out = a.clone(), torch.empty_like(a)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            p.row_fft_raw(x, conj_in=True, scale=0.5, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for src, want in ((a, eager[0]), (b, eager[1])):
        x.copy_(src)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want)


def test_the_raw_entry_refuses_bad_arguments(gpu):
    from tensor_cuda_fft_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    rows, n = 4, 64
    x = torch.from_numpy(rand_c64((rows + 1, n), 3)).to(gpu)
    out = torch.full((rows + 1, n), 7.0, dtype=torch.complex64, device=gpu)
    xi, oi = x.data_ptr(), out.data_ptr()
    assert xi % 16 == 0 and oi % 16 == 0
    INV, UNS = _lib.SMX_ERR_INVALID, _lib.SMX_ERR_UNSUPPORTED
    cases = [((xi, oi, -1, n, 0, 1.0, 0, s), INV), ((xi, oi, rows, n, 0, 1.0, -1, s), INV),
             ((xi, oi, rows, n, 16, 1.0, 0, s), INV), ((xi, oi, rows, n, -1, 1.0, 0, s), INV),
             ((None, oi, rows, n, 0, 1.0, 0, s), INV), ((xi, None, rows, n, 0, 1.0, 0, s), INV),
             ((xi + 8, oi, rows, n, 0, 1.0, 0, s), INV), ((xi, oi + 8, rows, n, 0, 1.0, 0, s), INV),
             ((xi, oi, rows, n, 0, float("inf"), 0, s), INV), ((xi, oi, rows, n, 0, float("nan"), 0, s), INV)]
    cases += [((xi, oi, rows, bad, 0, 1.0, 0, s), UNS) for bad in (3, 12, 8192, 0)]
    for args, want in cases:
        L.smx_rowfft(xi, oi, 0, n, 0, 1.0, 0, s)                       # a success in between leaves the next text to the refusal
        assert L.smx_rowfft(*args) == want, args
        assert L.smx_last_error(), args
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                    # nothing was enqueued
    assert L.smx_rowfft(xi, oi, 0, n, 0, 1.0, 0, s) == 0               # rows == 0: success, nothing enqueued
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(_lib.SmxError):
        pkg().row_fft_raw(torch.zeros(4, 12, dtype=torch.complex64, device=gpu))
    assert L.smx_rowfft(xi, oi, rows, n, 0, 1.0, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((out[rows] == 7.0).all()) and not bool((out[:rows] == 7.0).any())


@pytest.mark.parametrize("shape", [(3, 64), (2, 4096)])
def test_autograd_against_torch_fft_in_float64(gpu, shape):
    p = pkg()
    z, w = rand_c64(shape, 31), rand_c64(shape, 32)
    for ours, theirs in ((p.row_fft, torch.fft.fft), (p.row_ifft, torch.fft.ifft)):
        a = torch.from_numpy(z).to(gpu).requires_grad_()
        y = ours(a)
        (torch.from_numpy(w).to(gpu) * y).real.sum().backward()
        b = torch.from_numpy(z.astype(np.complex128)).requires_grad_()
        y64 = theirs(b, dim=-1)
        (torch.from_numpy(w.astype(np.complex128)) * y64).real.sum().backward()
        ef, eg = rel_err(y.detach().cpu().numpy(), y64.detach().numpy()), rel_err(a.grad.cpu().numpy(), b.grad.numpy())
        print(f"{ours.__name__} {shape}: forward {ef:.2e}, gradient {eg:.2e}; bound {TOL_ACT:.0e}")
        assert ef <= TOL_ACT and eg <= TOL_ACT, (ours.__name__, ef, eg)


def test_unsupported_lengths_on_the_device_run_the_sequence_transform(gpu):
    p = pkg()
    z = rand_c64((5, 100), 41)
    a = torch.from_numpy(z).to(gpu).requires_grad_()
    y = p.row_ifft(p.row_fft(a))
    y.real.sum().backward()
    assert rel_err(y.detach().cpu().numpy(), z.astype(np.complex128)) <= TOL_ACT
    assert rel_err(a.grad.cpu().numpy(), np.ones_like(z, dtype=np.complex128)) <= TOL_ACT


@pytest.mark.parametrize("shape", [(5, 4096), (48, 64, 32), (3, 512)])
def test_fftn_and_ifftn_through_the_row_transform(gpu, shape):
    p = pkg()
    z = rand_c64(shape, sum(shape))
    dev = torch.from_numpy(z).to(gpu)
    z64 = z.astype(np.complex128)
    fwd, inv = p.fftn(dev), p.ifftn(dev)
    assert fwd.dtype == torch.complex64 and tuple(fwd.shape) == shape and tuple(inv.shape) == shape
    errs = {"fftn": rel_err(fwd.cpu().numpy(), np.fft.fftn(z64)), "ifftn": rel_err(inv.cpu().numpy(), np.fft.ifftn(z64)),
            "ifftn(fftn(z))": rel_err(p.ifftn(fwd).cpu().numpy(), z64)}
    print(f"{shape}: max-normalised distances to float64 {errs}; bound {TOL_ACT:.0e}")
    assert max(errs.values()) <= TOL_ACT, errs
    assert torch.equal(dev, torch.from_numpy(z).to(gpu))               # the input is left as it was


def test_sst_round_trip_and_ifft_last_real(gpu):
    p = pkg()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((64, 128)).astype(np.float32)
    t = p.sst(torch.from_numpy(x).to(gpu), sparsity=1.0)
    back = t.to_spatial()
    assert back.dtype == torch.float32 and tuple(back.shape) == (64, 128)
    e1 = rel_err(back.cpu().numpy(), x.astype(np.float64))
    w = rand_c64((7, 256), 6)
    from tensor_cuda_fft_amd.frequency_ops import ifft_last_real
    got = ifft_last_real(torch.from_numpy(w).to(gpu))
    assert got.dtype == torch.float32
    e2 = rel_err(got.cpu().numpy(), np.fft.ifft(w.astype(np.complex128), axis=-1).real)
    print(f"sst(x).to_spatial() against x {e1:.2e}; ifft_last_real against float64 {e2:.2e}; bound {TOL_ACT:.0e}")
    assert e1 <= TOL_ACT and e2 <= TOL_ACT


def test_the_callers_dispatch(gpu, monkeypatch):
    """one native row launch per fftn where the last length is supported, none elsewhere"""
    p, f = pkg(), fnmod()
    calls = []
    real = f.row_fft_raw

    def spy(x, **kw):
        calls.append((tuple(x.shape), kw))
        return real(x, **kw)
    monkeypatch.setattr(f, "row_fft_raw", spy)
    p.fftn(torch.from_numpy(rand_c64((5, 4096), 1)).to(gpu))
    assert len(calls) == 1 and calls[0][0] == (5, 4096)
    p.ifftn(torch.from_numpy(rand_c64((5, 4096), 1)).to(gpu))
    assert len(calls) == 2 and calls[1][1].get("conj_out") and calls[1][1]["scale"] == 1.0 / (5 * 4096)
    del calls[:]
    p.fftn(torch.from_numpy(rand_c64((5, 100), 2)).to(gpu))
    p.ifftn(torch.from_numpy(rand_c64((5, 100), 2)).to(gpu))
    assert calls == []
    from tensor_cuda_fft_amd.frequency_ops import ifft_last_real
    ifft_last_real(torch.from_numpy(rand_c64((7, 256), 3)).to(gpu))
    assert len(calls) == 1 and calls[0][1] == {"conj_in": True, "real_out": True, "scale": 1.0 / 256}
