"""EnhancedSpectralBlock and its members without a GPU (reference fft_tensor/spectral_enhancements.py :20-71, :74-116,
:169-211, :278-333): exports, state_dict parity with the reference's own (tests/golden/E*.npz), the members' torch
composition against the reference's outputs, the reference's failures, and the C ABI surface of the row kernels."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, TOL_ACT, TOL_PARAM, load_golden, rel_err

T = torch.from_numpy
NEW_SYMBOLS = ("smx_enh_supported", "smx_enh_workspace_bytes", "smx_rope_norm_forward", "smx_rope_norm_backward",
               "smx_residual_norm_forward", "smx_residual_norm_backward", "smx_gate_blend_forward",
               "smx_gate_blend_backward")
BLOCKS = ["E01_enh_2x256x32", "E02_enh_2x100x16", "E03_enh_1x1024x8", "E04_enh_3x40x6"]


def _pkg():
    import tensor_cuda_fft_amd as pkg
    return pkg


def _sd(z):
    return {k[3:]: T(v) for k, v in z.items() if k.startswith("sd.")}


def test_names_are_exported():
    pkg = _pkg()
    for n in ("RotaryFrequencyEmbedding", "GatedSpectralUnit", "CausalFrequencyMask", "EnhancedSpectralBlock"):
        assert n in pkg.__all__ and hasattr(pkg, n)


@pytest.mark.parametrize("name", BLOCKS)
def test_block_state_dict_matches_the_reference(name):
    pkg = _pkg()
    z = load_golden(name)
    blk = pkg.EnhancedSpectralBlock(z["x"].shape[2], dropout=0.0)
    sd = _sd(z)
    assert list(blk.state_dict().keys()) == list(sd.keys())
    # the rotation table is built exactly as the reference builds it: bit for bit
    assert blk.rope.rotation.dtype == torch.complex64
    assert torch.equal(blk.rope.rotation, sd["rope.rotation"])
    assert torch.equal(blk.rope.inv_freq, sd["rope.inv_freq"])
    blk.load_state_dict(sd, strict=True)
    assert isinstance(blk.dropout, torch.nn.Dropout) and blk.gated.num_gates == 8


def _module_vs_fixture(m, z, tol=TOL_ACT):
    m.load_state_dict(_sd(z), strict=True)
    x = T(z["x"]).requires_grad_(True)
    y = m(x)
    y.backward(T(z["g"]))
    assert rel_err(y.detach().numpy(), z["y"]) <= tol
    assert rel_err(x.grad.numpy(), z["grad_x"]) <= tol
    for k, p in m.named_parameters():
        assert rel_err(p.grad.numpy(), z["grad." + k]) <= TOL_PARAM, k


def test_rope_on_cpu_matches_the_reference():
    z = load_golden("E11_rope_2x300x34")
    _module_vs_fixture(_pkg().RotaryFrequencyEmbedding(34), z)


def test_gated_unit_on_cpu_matches_the_reference():
    z = load_golden("E21_gsu_2x64x24")
    _module_vs_fixture(_pkg().GatedSpectralUnit(24), z)


def test_causal_mask_on_cpu_matches_the_reference():
    z = load_golden("E31_causal_2x50x8")
    m = _pkg().CausalFrequencyMask()
    assert m.causal_window.shape == (4096,) and float(m.causal_window.sum()) == 2048.0
    _module_vs_fixture(m, z)


def test_reference_failures_are_runtime_errors():
    pkg = _pkg()
    with pytest.raises(RuntimeError):
        pkg.RotaryFrequencyEmbedding(7)(torch.randn(1, 4, 7))
    with pytest.raises(RuntimeError):
        pkg.RotaryFrequencyEmbedding(8, max_seq_len=16)(torch.randn(1, 17, 8))
    with pytest.raises(RuntimeError):
        pkg.EnhancedSpectralBlock(7)(torch.randn(1, 4, 7))
    blk = pkg.EnhancedSpectralBlock(8)
    blk.rope = pkg.RotaryFrequencyEmbedding(8, max_seq_len=32)
    with pytest.raises(RuntimeError):
        blk(torch.randn(1, 33, 8))


def _declared():
    src = open(os.path.join(ROOT, "include", "smx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(smx_[a-z_0-9]+)\s*\(", src))


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    import subprocess
    from tensor_cuda_fft_amd import _lib
    declared = _declared()
    for n in NEW_SYMBOLS:
        assert n in declared and n in _lib._SIGS, n
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    h = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(h, n), n


def test_supported_widths_and_argument_checks():
    """No launch happens on any of these paths: they fail validation first."""
    from tensor_cuda_fft_amd import _lib
    L = _lib.lib()
    assert [bool(L.smx_enh_supported(d)) for d in (0, 2, 6, 7, 256, 1024, 1026)] == \
        [False, True, True, False, True, True, False]
    import ctypes
    nb = ctypes.c_size_t()
    assert L.smx_enh_workspace_bytes(4, 512, 256, ctypes.byref(nb)) == 0 and nb.value > 0
    # odd D, T beyond the table, misaligned pointer: refused before any launch
    assert L.smx_rope_norm_forward(16, 16, 8, None, None, None, None, 1e-5, 1e-5, 16, 16, 16, 1, 4, 7, 1, 0.0, None,
                                   None) == -2
    assert L.smx_rope_norm_forward(16, 16, 8, None, None, None, None, 1e-5, 1e-5, 16, 16, 16, 1, 9, 8, 1, 0.0, None,
                                   None) == -1
    assert L.smx_residual_norm_forward(20, 16, None, None, 1e-5, 16, 16, 16, 1, 4, 8, 0.0, None, None) == -1
    assert L.smx_gate_blend_forward(16, 16, None, None, None, 1e-5, 16, 16, 1, 4, 8, 1.5, None, None) == -1
