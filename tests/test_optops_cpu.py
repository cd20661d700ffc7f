"""fft_tensor.optimized_ops / production_ready on the CPU path against the reference's recorded results (tests/golden/O*,
made by tests/golden/make_golden_optops.py), the signatures, the strict state_dict load, the autograd definition of
bin_contract and the new header's ABI table.

Bound: 1e-6 max-normalised against the reference's own fp32 results (the bound of the sparse-tensor goldens): the CPU
path runs the reference's op sequence on the same torch kernels.  Measured distances when this file was written: 0.0 for
all seven convolutions and for every member (sparse FFT, matmul, the linear layer's forward and gradients, compress,
block_streaming_matmul, smart_conv2d, the cached to_spatial); each test prints its own."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import optops_common as oc
from conftest import GOLDEN, load_golden, rel_err

import tensor_cuda_fft_amd as pkg
from tensor_cuda_fft_amd import _lib, functional as fn, optimized_ops, production_ready

O = pkg.OptimizedFrequencyOps
BOUND = 1e-6


@pytest.fixture(scope="module")
def rec():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fcib" and v.ndim else v)
            for k, v in load_golden("O20_optops_members").items()}


def close(name, got, want):
    e = rel_err(got.detach().numpy(), want.numpy() if isinstance(want, torch.Tensor) else want)
    print(f"{name}: distance to the reference's result {e:.2e}")
    assert e <= BOUND, (name, e)


def test_exports():
    for name in ("bin_contract", "OptimizedFrequencyOps", "ProductionFrequencyLinear", "ProductionFrequencyOps",
                 "OptimizedSparseSpectralTensor"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    for mod in (optimized_ops, production_ready):
        assert not [n for n in vars(mod) if n.startswith("benchmark")]
        assert "print(" not in open(mod.__file__).read()


@pytest.mark.parametrize("i", range(len(oc.CONV1D)))
def test_conv1d_equals_the_reference(i):
    case = oc.CONV1D[i]
    g = load_golden(oc.conv1d_name(i))
    x, w = oc.conv1d_inputs(case)
    assert float(x.double().sum()) == float(g["x_sum"]) and float(w.double().sum()) == float(g["w_sum"])
    out = O.fast_frequency_conv1d(x, w, stride=case[6], padding=case[5])
    close(oc.conv1d_name(i), out, g["out"])
    e = rel_err(g["out"], oc.conv1d_def(x, w, case[6], case[5]).numpy())
    assert abs(e - float(g["ref_err"])) <= 1e-9 and e <= 5e-6         # the definition is the one the goldens were held against


@pytest.mark.parametrize("i", range(len(oc.CONV2D)))
def test_conv2d_equals_the_reference(i):
    case = oc.CONV2D[i]
    g = load_golden(oc.conv2d_name(i))
    x, w = oc.conv2d_inputs(case)
    assert float(x.double().sum()) == float(g["x_sum"]) and float(w.double().sum()) == float(g["w_sum"])
    out = O.fast_frequency_conv2d(x, w, stride=case[8], padding=case[7])
    close(oc.conv2d_name(i), out, g["out"])
    e = rel_err(g["out"], oc.conv2d_def(x, w, case[8], case[7]).numpy())
    assert abs(e - float(g["ref_err"])) <= 1e-9 and e <= 5e-6


def test_small_kernels_take_the_other_branch():
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 3, 100, generator=g), torch.randn(4, 3, 64, generator=g)
    assert torch.equal(O.fast_frequency_conv1d(x, w, 2, 3), torch.nn.functional.conv1d(x, w, stride=2, padding=3))
    x, w = torch.randn(2, 3, 12, 13, generator=g), torch.randn(4, 3, 7, 7, generator=g)
    assert torch.equal(O.fast_frequency_conv2d(x, w, (2, 1), 1), torch.nn.functional.conv2d(x, w, stride=(2, 1), padding=1))


def test_topk_and_sparse_fft(rec):
    v, i = O.fast_topk_sparse(rec["topk.data"], int(rec["topk.k"]))
    assert i.dtype == torch.int64 and torch.equal(i, rec["topk.indices"]) and torch.equal(v, rec["topk.values"])
    for p, shape in (("", (8, 12)), ("real.", (5, 9))):
        c, idx = O.optimized_sparse_fft(rec[f"sfft.{p}x"], 0.25 if not p else 0.2)
        assert torch.equal(idx, rec[f"sfft.{p}indices"])
        close(f"sfft.{p}coeffs", c, rec[f"sfft.{p}coeffs"])
        only = O.optimized_sparse_fft(rec[f"sfft.{p}x"], 0.25 if not p else 0.2, return_indices=False)
        assert torch.equal(only, c)
        close(f"sifft.{p}out", O.optimized_sparse_ifft(c, idx, shape, device="cpu"), rec[f"sifft.{p}out"])


def test_matmul(rec):
    out = O.fast_frequency_matmul(rec["matmul.x"], rec["matmul.w_freq"])
    close("matmul", out, rec["matmul.out"])
    close("matmul, block_size on a small weight", O.fast_frequency_matmul(rec["matmul.x"], rec["matmul.w_freq"], 8),
          rec["matmul.out"])
    with pytest.raises(AssertionError, match="Dimension mismatch: 12 != 11"):
        O.fast_frequency_matmul(rec["matmul.x"], rec["matmul.w_freq"][:11])


def test_linear_loads_a_reference_state_dict_strictly(rec):
    state = {k[len("linear.state."):]: v for k, v in rec.items() if k.startswith("linear.state.")}
    assert sorted(state) == ["bias", "weight_freq", "weight_indices"]
    lin = pkg.ProductionFrequencyLinear(48, 10, sparsity=0.25)
    assert list(lin.state_dict()) == list(state)
    lin.load_state_dict(state, strict=True)
    y = lin(rec["linear.x"])
    close("linear.out", y, rec["linear.out"])
    y.backward(rec["linear.g"])
    close("linear.grad_weight_freq", lin.weight_freq.grad, rec["linear.grad_weight_freq"])
    close("linear.grad_bias", lin.bias.grad, rec["linear.grad_bias"])


def test_linear_draws_what_the_reference_draws_and_caches_as_it_does(rec):
    torch.manual_seed(int(rec["linear.seed"]))
    lin = pkg.ProductionFrequencyLinear(48, 10, sparsity=0.25)
    assert torch.equal(lin.weight_indices, rec["linear.state.weight_indices"])
    assert torch.equal(lin.weight_freq.detach(), rec["linear.state.weight_freq"])
    assert pkg.ProductionFrequencyLinear(8, 4, bias=False).bias is None
    x = rec["linear.x"]
    assert lin._materialize_weights() is not lin._materialize_weights()          # training: nothing is kept
    lin.eval()
    w = lin._materialize_weights()
    assert lin._materialize_weights() is w
    with torch.no_grad():
        lin.weight_freq.mul_(2.0)
    assert lin._materialize_weights() is w                                       # stale until told
    lin.invalidate_cache()
    assert torch.allclose(lin._materialize_weights(), 2.0 * w)
    assert lin(x).shape == (3, 7, 10)


def test_production_ops(rec):
    P = pkg.ProductionFrequencyOps
    if not torch.cuda.is_available():                      # compress_tensor has the reference's device: 'cuda', else the CPU
        with pytest.warns(UserWarning, match="CUDA not available"):
            comp = P.compress_tensor(rec["compress.x"], sparsity=float(rec["compress.sparsity"]))
        assert isinstance(comp, pkg.SparseSpectralTensor)
        assert torch.equal(comp.indices, rec["compress.indices"].long())
        close("compress.freq_coeffs", comp.freq_coeffs, rec["compress.freq_coeffs"])
        close("compress.to_spatial", comp.to_spatial(), rec["compress.to_spatial"])
    comp = pkg.SparseSpectralTensor(data=rec["compress.x"], sparsity=float(rec["compress.sparsity"]), device="cpu")
    close("bsm.out", P.block_streaming_matmul(rec["bsm.x"], comp, block_size=int(rec["bsm.block_size"])), rec["bsm.out"])
    close("smart.out", P.smart_conv2d(rec["smart.x"], rec["smart.w"], padding=1), rec["smart.out"])


def test_cached_sparse_tensor(rec):
    o = pkg.OptimizedSparseSpectralTensor(data=rec["compress.x"], sparsity=float(rec["compress.sparsity"]), device="cpu")
    first = o.to_spatial()
    close("osst.to_spatial", first, rec["osst.to_spatial"])
    assert o.to_spatial() is first
    o.invalidate_cache()
    again = o.to_spatial()
    assert again is not first and torch.equal(again, first)
    doubled = o * 2.0                                       # a derived tensor starts without the parent's cache
    assert isinstance(doubled, pkg.OptimizedSparseSpectralTensor)
    assert torch.allclose(doubled.to_spatial(), 2.0 * first, atol=1e-5)


def _signature(cls, name):
    f = inspect.getattr_static(cls, name)
    return str(inspect.signature(getattr(f, "__func__", f)))


def test_signatures_are_the_reference_s(rec):
    recorded = [str(s) for s in rec["signatures"]]
    assert len(recorded) == sum(len(v) for v in oc.MEMBERS.values())

    def plain(s):                                          # the sparse tensor's class lives in another module here
        return re.sub(r"[\w.]+\.SparseSpectralTensor", "SparseSpectralTensor", s)
    it = iter(recorded)
    for cls, names in oc.MEMBERS.items():
        for n in names:
            want, got = plain(next(it)), plain(f"{cls}.{n}{_signature(getattr(pkg, cls), n)}")
            if " -> " not in want:                         # (the reference's scripted fast_topk_sparse records no result type)
                got = got.split(" -> ")[0]
            assert got == want


def test_bin_contract_definition_and_its_gradients():
    g = torch.Generator().manual_seed(3)
    x = torch.complex(torch.randn(2, 3, 4, generator=g, dtype=torch.float64), torch.randn(2, 3, 4, generator=g, dtype=torch.float64))
    w = torch.complex(torch.randn(3, 4, 5, generator=g, dtype=torch.float64), torch.randn(3, 4, 5, generator=g, dtype=torch.float64))
    x.requires_grad_(), w.requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: fn.bin_contract(a, b), (x, w))
    gy = torch.complex(torch.randn(2, 3, 5, generator=g, dtype=torch.float64), torch.randn(2, 3, 5, generator=g, dtype=torch.float64))
    gx, gw = torch.autograd.grad(fn.bin_contract(x, w), (x, w), gy)
    dx, dw = oc.bin_contract_grads_def(x.detach(), w.detach(), gy)          # the formulas of smx_fconv.h
    assert torch.allclose(gx, dx, rtol=0, atol=1e-12) and torch.allclose(gw, dw, rtol=0, atol=1e-12)
    assert torch.equal(fn.bin_contract(x.detach(), w.detach()), oc.bin_contract_def(x.detach(), w.detach()))
    with pytest.raises(ValueError, match="need \\(B, P, Ci\\) and \\(P, Ci, Co\\)"):
        fn.bin_contract(x, w[:2])
    with pytest.raises(ValueError, match="max_workgroups"):
        fn.bin_contract(x, w, max_workgroups=-1)
    assert fn.bin_contract(x[:0], w).shape == (0, 3, 5)


def test_the_new_header_is_part_of_the_abi_and_bound_from_its_own_table():
    import ctypes
    inc = os.path.dirname(_lib.HEADER_PATH)
    assert '#include "smx_fconv.h"' in open(_lib.HEADER_PATH).read()
    text = open(os.path.join(inc, "smx_fconv.h")).read()
    table = _lib._SIGS_MORE["smx_fconv.h"]
    entries = ("smx_bin_contract_backward", "smx_bin_contract_forward", "smx_bin_contract_supported")
    assert tuple(sorted(table)) == entries
    for e in entries:
        assert f"int {e}(" in text and e not in _lib._SIGS and e not in _lib._SIGS_EXT and e not in _lib._SINCE
    assert _lib.SMX_VERSION == 303
    codes = {ctypes.c_int: "i", ctypes.c_longlong: "q", ctypes.c_float: "f", ctypes.c_void_p: "P", ctypes.c_size_t: "z"}

    def spell(t):
        return codes[t] if t in codes else "[" + codes[t._type_] + "]"
    got = [f"{n} {spell(r)}({''.join(spell(a) for a in args)})" for n, (r, args) in sorted(table.items())]
    got += [f"const {n} {v}" for n, v in sorted(_lib._DEFINES_MORE["smx_fconv.h"].items())]
    assert got == open(os.path.join(GOLDEN, "abi_signatures_fconv.txt")).read().splitlines()
    if os.path.exists(_lib.LIB_PATH):
        for e in entries:
            assert getattr(_lib.lib(), e).argtypes == table[e][1]
        assert _lib.lib().smx_bin_contract_supported(8, 4097, 64, 64) == 1
        assert _lib.lib().smx_bin_contract_supported(8, 2 ** 31, 64, 64) == 0
        assert _lib.lib().smx_bin_contract_supported(0, 1, 1, 1) == 0
