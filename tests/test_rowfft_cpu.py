"""The row transform's host side: the new header in the binding and its recorded table, row_fft / row_ifft and fftn / ifftn
on CPU tensors (torch.fft, bit for bit, with torch's gradients), and the errors row_fft_raw raises before any launch."""
import ctypes
import os

import pytest
import torch

from conftest import GOLDEN

import tensor_cuda_fft_amd as pkg
from tensor_cuda_fft_amd import _lib, functional as fn


def test_exports():
    for name in ("rowfft_supported", "row_fft_raw", "row_fft", "row_ifft"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(fn, name), name


def test_the_new_header_is_part_of_the_abi_and_bound_from_its_own_table():
    inc = os.path.dirname(_lib.HEADER_PATH)
    smx_h = open(_lib.HEADER_PATH).read()
    assert '#include "smx_rowfft.h"' in smx_h and smx_h.index('"smx_quant.h"') < smx_h.index('"smx_rowfft.h"')
    assert "smx_rowfft.h" in _lib.MORE_HEADERS
    text = open(os.path.join(inc, "smx_rowfft.h")).read()
    table = _lib._SIGS_MORE["smx_rowfft.h"]
    entries = ("smx_rowfft", "smx_rowfft_supported")
    assert tuple(sorted(table)) == entries
    for e in entries:
        assert f"int {e}(" in text and e not in _lib._SIGS and e not in _lib._SIGS_EXT and e not in _lib._SINCE
        assert all(e not in t for h, t in _lib._SIGS_MORE.items() if h != "smx_rowfft.h")
    codes = {ctypes.c_int: "i", ctypes.c_longlong: "q", ctypes.c_float: "f", ctypes.c_void_p: "P", ctypes.c_size_t: "z"}

    def spell(t):
        return codes[t] if t in codes else "[" + codes[t._type_] + "]"
    got = [f"{n} {spell(r)}({''.join(spell(a) for a in args)})" for n, (r, args) in sorted(table.items())]
    got += [f"const {n} {v}" for n, v in sorted(_lib._DEFINES_MORE["smx_rowfft.h"].items())]
    assert got == open(os.path.join(GOLDEN, "abi_signatures_rowfft.txt")).read().splitlines()
    # the flag constants are the header's
    assert (_lib.SMX_ROWFFT_CONJ_IN, _lib.SMX_ROWFFT_CONJ_OUT, _lib.SMX_ROWFFT_REAL_IN, _lib.SMX_ROWFFT_REAL_OUT) == (1, 2, 4, 8)
    assert _lib.SMX_ROWFFT_MAX_N == fn.ROWFFT_MAX_N == 4096
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        for e in entries:
            assert getattr(L, e).argtypes == table[e][1]
        assert [n for n in range(0, 8200) if L.smx_rowfft_supported(n)] == [2 ** i for i in range(1, 13)]
        assert fn.rowfft_supported(4096) and not fn.rowfft_supported(8192) and not fn.rowfft_supported(12)
        # a zero-sized call succeeds without pointers; bad arguments are refused before anything is touched
        assert L.smx_rowfft(None, None, 0, 64, 0, 1.0, 0, None) == 0
        assert L.smx_rowfft(None, None, -1, 64, 0, 1.0, 0, None) == _lib.SMX_ERR_INVALID and L.smx_last_error()
        assert L.smx_rowfft(None, None, 0, 12, 0, 1.0, 0, None) == _lib.SMX_ERR_UNSUPPORTED and L.smx_last_error()
        assert L.smx_rowfft(None, None, 4, 64, 0, 1.0, 0, None) == _lib.SMX_ERR_INVALID


@pytest.mark.parametrize("shape", [(3, 64), (2, 5, 12), (7,)])
def test_row_fft_and_row_ifft_on_the_cpu_are_torch_fft_with_its_gradients(shape):
    g = torch.Generator().manual_seed(sum(shape))
    z = torch.randn(shape, dtype=torch.complex64, generator=g)
    w = torch.randn(shape, dtype=torch.complex64, generator=g)
    for ours, theirs in ((pkg.row_fft, torch.fft.fft), (pkg.row_ifft, torch.fft.ifft)):
        assert torch.equal(torch.view_as_real(ours(z)), torch.view_as_real(theirs(z, dim=-1)))
        a, b = z.clone().requires_grad_(), z.clone().requires_grad_()
        (w * ours(a)).real.sum().backward()
        (w * theirs(b, dim=-1)).real.sum().backward()
        assert torch.equal(torch.view_as_real(a.grad), torch.view_as_real(b.grad))
    with pytest.raises(TypeError):
        pkg.row_fft(z.real)
    with pytest.raises(TypeError):
        pkg.row_ifft(z.to(torch.complex128))


def test_row_fft_raw_refuses_what_it_cannot_run():
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        pkg.row_fft_raw(torch.zeros(4, 8, dtype=torch.complex64))
    with pytest.raises(TypeError):
        pkg.row_fft_raw([1.0, 2.0])
    with pytest.raises(TypeError, match="complex64 or float32"):                 # dtype and rank are checked before the device
        pkg.row_fft_raw(torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="at least one dimension"):
        pkg.row_fft_raw(torch.zeros((), dtype=torch.complex64))
    with pytest.raises(ValueError, match="max_workgroups"):
        pkg.row_fft_raw(torch.zeros(4, 8, dtype=torch.complex64), max_workgroups=-1)


@pytest.mark.parametrize("shape", [(5, 4096), (6, 10, 4), (9,), (1, 7, 1)])
def test_fftn_and_ifftn_on_the_cpu_are_still_torch_fft(shape):
    g = torch.Generator().manual_seed(sum(shape))
    z = torch.randn(shape, dtype=torch.complex64, generator=g)
    assert torch.equal(torch.view_as_real(pkg.fftn(z)), torch.view_as_real(torch.fft.fftn(z)))
    assert torch.equal(torch.view_as_real(pkg.ifftn(z)), torch.view_as_real(torch.fft.ifftn(z)))
    assert torch.equal(torch.view_as_real(fn.fftn_real(z.real.contiguous())),
                       torch.view_as_real(torch.fft.fftn(z.real.to(torch.complex64))))
    assert torch.equal(fn.ifftn_real(z), torch.fft.ifftn(z).real)
