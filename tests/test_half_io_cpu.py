"""bf16 / fp16 activations: the C ABI surface and the plan coverage of the native 2-byte I/O, without a GPU."""
import os
import re

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "smx.h")
NEW = ("smx_io_supported", "smx_forward_io", "smx_backward_io")


@pytest.fixture(scope="module")
def L():
    import subprocess
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


def test_header_declares_the_io_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for macro, v in (("SMX_IO_F32", 0), ("SMX_IO_BF16", 1), ("SMX_IO_F16", 2)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(v) + r"\b", src), macro
    from tensor_cuda_fft_amd import _lib
    for name in NEW:
        assert name in _lib._SIGS and _lib._SINCE[name] == 303


@pytest.mark.parametrize("io", [1, 2])
@pytest.mark.parametrize("shape", [(64, 4096, 256, 128),       # C2: k_fused, one band
                                   (8, 65536, 256, 128),       # C3: residue split
                                   (64, 4096, 512, 256),       # two bands
                                   (2, 4096, 8, 300),          # four bands
                                   (8, 512, 256, 128)])        # C1
def test_native_on_the_streaming_plans(L, shape, io):
    assert L.plan(*shape).path == L.SMX_PATH_DECIMATED
    assert L.lib().smx_io_supported(*shape, io) == 1
    assert L.io_supported(*shape, io)


@pytest.mark.parametrize("io", [1, 2])
@pytest.mark.parametrize("shape", [(2, 1000, 8, 4),            # direct plan
                                   (2, 4096, 8, 600),          # more than 512 bins: four-step
                                   (2, 8704, 8, 600),          # more than 512 bins: band groups
                                   (2, 512, 7, 4),             # odd D
                                   (2, 4112, 8, 64)])          # sixteen-row plan
def test_up_cast_route_elsewhere(L, shape, io):
    assert L.lib().smx_io_supported(*shape, io) == 0


def test_f32_is_native_everywhere_and_bad_io_is_refused(L):
    lib = L.lib()
    assert lib.smx_io_supported(2, 1000, 8, 4, 0) == 1
    for io in (-1, 3, 7):
        assert lib.smx_io_supported(64, 4096, 256, 128, io) == 0
        rc = lib.smx_forward_io(None, None, None, None, None, None, None, 0, 2, 512, 8, 4, 0, 0.0, None, None,
                                None, io)
        assert rc != 0 and b"io must be" in lib.smx_last_error()
        rc = lib.smx_backward_io(None, None, None, None, None, None, None, None, None, 0, 2, 512, 8, 4, 7, 0.0,
                                 None, None, None, io)
        assert rc != 0 and b"io must be" in lib.smx_last_error()
    assert lib.smx_io_supported(0, 4096, 256, 128, 1) == 0       # invalid shape


def test_unsupported_plan_is_an_error_not_a_fallback(L):
    lib = L.lib()
    # validation and plan refusal happen before anything touches device memory
    rc = lib.smx_forward_io(16, 16, 16, None, 16, None, None, 0, 2, 1000, 8, 4, 0, 0.0, None, None, None, 1)
    assert rc == -2                                        # SMX_ERR_UNSUPPORTED
    assert b"smx_io_supported" in lib.smx_last_error()
    rc = lib.smx_backward_io(16, 16, 16, 16, 16, None, None, None, None, 0, 2, 1000, 8, 4, 2, 0.0, None, None,
                             None, 2)
    assert rc != 0 and b"smx_io_supported" in lib.smx_last_error()
    # 2-byte rows need 4-byte alignment
    rc = lib.smx_forward_io(18, 16, 16, None, 16, None, None, 0, 64, 4096, 256, 128, 0, 0.0, None, None, None, 1)
    assert rc != 0 and b"4-byte aligned" in lib.smx_last_error()


def test_half_dtypes_reach_the_library_checks_not_a_type_error():
    """fp64 still raises TypeError; bf16 / fp16 are accepted dtypes (a CPU tensor then fails on the device check)."""
    import torch
    from tensor_cuda_fft_amd import functional as fn
    w = torch.ones(8, 4)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            fn.spectral_mix(torch.zeros(2, 512, 8, dtype=dt), w, w)
    with pytest.raises((TypeError, RuntimeError)):
        fn.spectral_mix(torch.zeros(2, 512, 8, dtype=torch.float64), w, w)
