"""bf16 / fp16 activations of the causal spectral convolution: the C ABI surface (smx_conv_*_io) and which plans
run the 2-byte rows natively, without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "smx.h")
NEW = ("smx_conv_io_supported", "smx_conv_forward_io", "smx_conv_backward_io")


@pytest.fixture(scope="module")
def L():
    import subprocess
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


def _sh(L, B, R, D, n_fft):
    return ctypes.byref(L.smx_shape(B, R, D, n_fft // 2 + 1, n_fft, n_fft // 2 + 1))


def test_header_declares_the_conv_io_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert re.search(r"#define\s+SMX_VERSION\s+303\b", src)
    from tensor_cuda_fft_amd import _lib
    for name in NEW:
        assert name in _lib._SIGS and _lib._SINCE[name] == 303


NATIVE = [(64, 1024, 512, 2048),      # bench.py's f2 row: 32-channel workgroups
          (8, 1024, 512, 2048),       # fft_lm's default batch: 16-channel workgroups
          (32, 1920, 512, 2048),      # rows > n_fft / 2: folded
          (64, 768, 256, 1024),       # n_fft 1024
          (16, 256, 256, 512),        # n_fft 512, rows = n_fft / 2
          (16, 200, 512, 512),        # n_fft 512, rows < n_fft / 2
          (8, 511, 512, 512)]         # n_fft 512, folded with padding


@pytest.mark.parametrize("io", [0, 1, 2])
@pytest.mark.parametrize("shape", NATIVE)
def test_native_on_the_single_launch_plan(L, shape, io):
    assert L.lib().smx_conv_io_supported(_sh(L, *shape), io) == 1
    assert L.conv_io_supported(*shape, io)


@pytest.mark.parametrize("io", [1, 2])
@pytest.mark.parametrize("shape", [(4, 2048, 64, 4096),     # three-launch long convolution
                                   (8, 200, 64, 512),       # few work items: the three-launch plan
                                   (64, 1024, 511, 2048)])  # odd channel count: no convolution plan at all
def test_up_cast_route_elsewhere(L, shape, io):
    assert L.lib().smx_conv_io_supported(_sh(L, *shape), io) == 0
    assert L.lib().smx_conv_io_supported(_sh(L, *shape), 0) == L.lib().smx_conv_supported(_sh(L, *shape))


def test_conv1_option_off_means_no_native_rows(L):
    with L.options(conv1=0):
        assert not L.conv_io_supported(64, 1024, 512, 2048, 1)
        assert L.conv_io_supported(64, 1024, 512, 2048, 0)
    assert L.conv_io_supported(64, 1024, 512, 2048, 1)


def test_bad_io_unsupported_plan_and_misalignment_are_errors(L):
    lib = L.lib()
    sh = _sh(L, 64, 1024, 512, 2048)
    for io in (-1, 3):
        assert lib.smx_conv_io_supported(sh, io) == 0
        rc = lib.smx_conv_forward_io(sh, 16, 16, 16, None, 16, None, None, 0, io, None)
        assert rc != 0 and b"io must be" in lib.smx_last_error()
    # validation and plan refusal happen before anything touches device memory
    long_sh = _sh(L, 4, 2048, 64, 4096)
    rc = lib.smx_conv_forward_io(long_sh, 16, 16, 16, None, 16, None, None, 0, 1, None)
    assert rc == -2 and b"smx_conv_io_supported" in lib.smx_last_error()          # SMX_ERR_UNSUPPORTED
    rc = lib.smx_conv_backward_io(long_sh, 16, 16, 16, 16, None, 16, None, None, None, None, 0, 2, None)
    assert rc == -2 and b"smx_conv_io_supported" in lib.smx_last_error()
    with L.options(conv1=0):
        rc = lib.smx_conv_forward_io(sh, 16, 16, 16, None, 16, None, None, 0, 1, None)
        assert rc == -2 and b"smx_conv_io_supported" in lib.smx_last_error()
    rc = lib.smx_conv_forward_io(sh, 18, 16, 16, None, 16, None, None, 0, 1, None)
    assert rc != 0 and b"4-byte aligned" in lib.smx_last_error()
    rc = lib.smx_conv_backward_io(sh, 16, 16, 16, 16, None, 18, None, None, None, None, 0, 2, None)
    assert rc != 0 and b"4-byte aligned" in lib.smx_last_error()


def test_half_dtypes_reach_the_device_check_not_a_type_error():
    """bf16 / fp16 are accepted dtypes: a CPU tensor fails on the device check, not on its dtype."""
    import torch
    from tensor_cuda_fft_amd import functional as fn
    from tensor_cuda_fft_amd.fixed_spectral import causal_spectral_conv
    h = torch.ones(1025)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            fn.rank_one_conv(torch.zeros(8, 1024, 512, dtype=dt), h, h, None, 2048)
        for C in (512, 7):                        # the convolution's plan, and the spectral_filter route
            x = torch.zeros(2, 1024, C, dtype=dt)
            with pytest.raises(RuntimeError, match="no CPU implementation"):
                causal_spectral_conv(x, torch.zeros(128, dtype=dt), torch.ones(C, dtype=dt),
                                     torch.zeros(1025, dtype=dt), torch.ones(2, C, dtype=dt))
    # (on the CPU the device check comes first; tests/test_conv_half_io_gpu.py has fp64 on the device)
    with pytest.raises((TypeError, RuntimeError)):
        fn.rank_one_conv(torch.zeros(8, 1024, 512, dtype=torch.float64), h, h, None, 2048)
    with pytest.raises((TypeError, RuntimeError)):
        causal_spectral_conv(torch.zeros(2, 1024, 512, dtype=torch.float64), torch.zeros(128), torch.ones(512))
