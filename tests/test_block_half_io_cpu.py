"""bf16 / fp16 activations of the fused block line: the C ABI surface and the shapes with native 2-byte block rows,
without a GPU."""
import os
import re

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "smx.h")
NEW = ("smx_block_io_supported", "smx_block_forward_io", "smx_block_backward_io")


@pytest.fixture(scope="module")
def L():
    import subprocess
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


def test_header_declares_the_block_io_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
    from tensor_cuda_fft_amd import _lib
    for name in NEW:
        assert name in _lib._SIGS and _lib._SINCE[name] == 303


def test_library_exports_them_and_keeps_its_version(L):
    lib = L.lib()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.smx_version() == 303


@pytest.mark.parametrize("io", [1, 2])
@pytest.mark.parametrize("shape", [(64, 4096, 256, 128),       # one band
                                   (8, 1024, 64, 200),         # two bands
                                   (32, 1024, 128, 300)])      # four bands
def test_native_on_the_single_launch_plan(L, shape, io):
    p = L.plan(*shape)
    assert (p.path, p.nsplit, p.groups) == (L.SMX_PATH_DECIMATED, 1, 1)
    assert L.lib().smx_block_io_supported(*shape, io) == 1
    assert L.block_io_supported(*shape, io)


@pytest.mark.parametrize("io", [1, 2])
@pytest.mark.parametrize("shape", [(8, 65536, 256, 128),       # residue split
                                   (2, 1000, 8, 4),            # direct plan
                                   (2, 4112, 64, 64),          # sixteen-row plan
                                   (2, 4096, 64, 600),         # more than 512 bins
                                   (2, 512, 7, 4),             # odd D
                                   (8, 1024, 63, 32),          # odd D on a streaming length
                                   (0, 4096, 256, 128),        # invalid shapes
                                   (64, 4096, 0, 128),
                                   (64, 4096, 256, 0)])
def test_up_cast_route_elsewhere(L, shape, io):
    assert L.lib().smx_block_io_supported(*shape, io) == 0


def test_f32_equals_block_supported_and_bad_io_is_refused(L):
    lib = L.lib()
    for shape in ((64, 4096, 256, 128), (2, 1000, 8, 4), (2, 512, 7, 4), (2, 512, 8192, 4), (2, 512, 4100, 4)):
        assert lib.smx_block_io_supported(*shape, 0) == lib.smx_block_supported(shape[2]), shape
    for io in (-1, 3, 7):
        assert lib.smx_block_io_supported(64, 4096, 256, 128, io) == 0
        rc = lib.smx_block_forward_io(None, None, None, 1e-5, None, None, None, None, None, None, None, 0,
                                      64, 4096, 256, 128, 0.0, None, None, None, io)
        assert rc != 0 and b"io must be" in lib.smx_last_error()
        rc = lib.smx_block_backward_io(*([None] * 15), 0, 64, 4096, 256, 128, 7, 0.0, None, None, None, io)
        assert rc != 0 and b"io must be" in lib.smx_last_error()


@pytest.mark.parametrize("io", [1, 2])
def test_unsupported_plan_is_an_error_not_a_fallback(L, io):
    lib = L.lib()
    # validation and the plan refusal happen before anything touches device memory (the pointers are not memory)
    for shape in ((2, 1000, 8, 4), (8, 65536, 256, 128), (2, 512, 7, 4)):
        rc = lib.smx_block_forward_io(16, 16, 16, 1e-5, 16, 16, None, 32, None, 16, None, 0, *shape, 0.0, None,
                                      None, None, io)
        assert rc == -2 and b"smx_block_io_supported" in lib.smx_last_error(), shape      # SMX_ERR_UNSUPPORTED
        rc = lib.smx_block_backward_io(*([16] * 7), 32, *([16] * 6), None, 0, *shape, 7, 0.0, None, None, None, io)
        assert rc == -2 and b"smx_block_io_supported" in lib.smx_last_error(), shape
    # a native shape: grad_h is required, and the 2-byte rows want 8 bytes
    rc = lib.smx_block_backward_io(*([16] * 7), 32, *([16] * 5), None, None, 0, 64, 4096, 256, 128, 7, 0.0, None,
                                   None, None, io)
    assert rc != 0 and b"grad_h" in lib.smx_last_error()
    rc = lib.smx_block_forward_io(20, 16, 16, 1e-5, 16, 16, None, 32, None, 16, None, 0, 64, 4096, 256, 128, 0.0,
                                  None, None, None, io)
    assert rc != 0 and b"8-byte aligned" in lib.smx_last_error()


def test_half_dtypes_reach_the_library_checks_not_a_type_error():
    """fp64 still raises TypeError; bf16 / fp16 are accepted dtypes (a CPU tensor then fails on the device check)."""
    import torch
    from tensor_cuda_fft_amd import functional as fn
    w = torch.ones(8, 4)
    ln = torch.ones(8)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            fn.spectral_block_mix(torch.zeros(2, 512, 8, dtype=dt), ln, ln, 1e-5, w, w)
    with pytest.raises((TypeError, RuntimeError)):
        fn.spectral_block_mix(torch.zeros(2, 512, 8, dtype=torch.float64), ln, ln, 1e-5, w, w)
