"""fft_tensor.polar_quantization / zero_materialize / llamaizer (the offline half) on the CPU against the reference's
recorded results (tests/golden/R11.., made by tests/golden/make_golden_quant.py), the signatures, the strict state_dict
load, gradcheck and the new header's ABI table.

The quantisers run the reference's op sequence on the CPU: their codes and values are compared BIT for bit.  The
transform-based ops sum in another order (one GEMM, not a broadcast product), so they are held to TOL_ACT against the
reference's fp32 results; measured when this file was written: 1.3e-7 (layer forward), 4e-7 at most for the rest."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import quant_common as qc
from conftest import GOLDEN, TOL_ACT, load_golden, rel_err

import tensor_cuda_fft_amd as pkg
from tensor_cuda_fft_amd import _lib, functional as fn, llamaizer, polar_quantization, zero_materialize

C = pkg.ConvolutionTheoremMatMul
Q = pkg.LogarithmicQuantizer


def tensors(name):
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fcibu" and v.ndim else v) for k, v in load_golden(name).items()}


@pytest.fixture(scope="module")
def rec():
    return tensors("R31_zero_materialize")


def bits_equal(a, b):
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy().view(np.uint8), b.numpy().view(np.uint8))


def close(name, got, want):
    e = rel_err(got.detach().numpy(), want.numpy())
    print(f"{name}: distance to the reference's result {e:.2e}")
    assert e <= TOL_ACT, (name, e)


def test_exports():
    for name in ("polar_range", "polar_quantize", "polar_dequantize", "log8_encode", "log8_decode", "log8_encode_complex",
                 "log8_decode_complex", "PolarQuantizer", "ConvolutionTheoremMatMul", "WirtingerAutograd",
                 "FrequencyLinearLayer", "LogarithmicQuantizer", "frequency_linear", "frequency_conv1d", "FFTConverter"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    for mod in (polar_quantization, zero_materialize, llamaizer):
        assert "print(" not in open(mod.__file__).read()
    assert not hasattr(llamaizer, "FFTLlama")


def _signature(owner, name):
    f = inspect.getattr_static(owner, name) if isinstance(owner, type) else getattr(owner, name)
    return str(inspect.signature(getattr(f, "__func__", f)))


def test_signatures_are_the_reference_s(rec):
    recorded = [str(s) for s in rec["signatures"]]
    assert len(recorded) == sum(len(v) for v in qc.MEMBERS.values())

    def plain(s):                                          # the classes live in another package here
        return re.sub(r"[\w]+\.zero_materialize\.FrequencyLinearLayer", "FrequencyLinearLayer", s)
    it = iter(recorded)
    for cls, names in qc.MEMBERS.items():
        for n in names:
            owner = getattr(pkg, cls) if cls else zero_materialize
            assert plain(f"{cls}.{n}{_signature(owner, n)}") == plain(next(it))


def test_the_new_header_is_part_of_the_abi_and_bound_from_its_own_table():
    inc = os.path.dirname(_lib.HEADER_PATH)
    assert '#include "smx_quant.h"' in open(_lib.HEADER_PATH).read()
    assert "smx_quant.h" in _lib.MORE_HEADERS
    text = open(os.path.join(inc, "smx_quant.h")).read()
    table = _lib._SIGS_MORE["smx_quant.h"]
    entries = ("smx_log8_decode", "smx_log8_decode_c64", "smx_log8_encode", "smx_log8_encode_c64", "smx_polar_dequantize",
               "smx_polar_quantize", "smx_polar_range", "smx_polar_range_workspace_bytes")
    assert tuple(sorted(table)) == entries
    for e in entries:
        assert f"int {e}(" in text and e not in _lib._SIGS and e not in _lib._SIGS_EXT and e not in _lib._SINCE
        assert all(e not in t for h, t in _lib._SIGS_MORE.items() if h != "smx_quant.h")
    codes = {ctypes.c_int: "i", ctypes.c_longlong: "q", ctypes.c_float: "f", ctypes.c_void_p: "P", ctypes.c_size_t: "z"}

    def spell(t):
        return codes[t] if t in codes else "[" + codes[t._type_] + "]"
    got = [f"{n} {spell(r)}({''.join(spell(a) for a in args)})" for n, (r, args) in sorted(table.items())]
    got += [f"const {n} {v}" for n, v in sorted(_lib._DEFINES_MORE["smx_quant.h"].items())]
    assert got == open(os.path.join(GOLDEN, "abi_signatures_quant.txt")).read().splitlines()
    if os.path.exists(_lib.LIB_PATH):
        for e in entries:
            assert getattr(_lib.lib(), e).argtypes == table[e][1]
        need = ctypes.c_size_t(1)
        assert _lib.lib().smx_polar_range_workspace_bytes(0, ctypes.byref(need)) == 0 and need.value == 0
        assert _lib.lib().smx_polar_range_workspace_bytes(4099, ctypes.byref(need)) == 0 and need.value % 256 == 0 < need.value
        assert _lib.lib().smx_polar_range_workspace_bytes(-1, ctypes.byref(need)) == _lib.SMX_ERR_INVALID
        # zero-sized calls succeed without pointers; bad bit counts and sizes are refused before anything is touched
        assert _lib.lib().smx_polar_quantize(None, None, None, 0, 4, 8, 0.0, 1.0, 0, None) == 0
        assert _lib.lib().smx_log8_encode(None, None, 0, 0, None) == 0
        assert _lib.lib().smx_polar_quantize(None, None, None, 0, 0, 8, 0.0, 1.0, 0, None) == _lib.SMX_ERR_INVALID
        assert _lib.lib().smx_polar_dequantize(None, None, None, 0, 4, 9, 0.0, 1.0, 0, None) == _lib.SMX_ERR_INVALID
        assert _lib.lib().smx_polar_quantize(None, None, None, 5, 4, 8, 0.0, 1.0, 0, None) == _lib.SMX_ERR_INVALID
        assert _lib.lib().smx_log8_decode(None, None, -1, 0, None) == _lib.SMX_ERR_INVALID
        assert _lib.lib().smx_log8_decode_c64(None, None, None, 3, -1, None) == _lib.SMX_ERR_INVALID


# ---- the quantisers: the reference's bits -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", qc.POLAR_SHAPES)
@pytest.mark.parametrize("config", qc.POLAR_CONFIGS)
def test_polar_quantizer_gives_the_reference_s_bits(shape, config):
    g = tensors(qc.polar_name(shape))
    z = qc.polar_input(shape)
    assert complex(z.to(torch.complex128).sum()) == complex(g["z_sum"])
    c = "%d_%d" % config
    q = pkg.PolarQuantizer(*config)
    assert (q.mag_bits, q.phase_bits, q.mag_levels, q.phase_levels, q.mag_range) == (*config, 2 ** config[0], 2 ** config[1], None)
    with pytest.raises(TypeError):
        q.dequantize(g[f"mag_q.{c}"], g[f"phase_q.{c}"])
    mag_q, phase_q = q.quantize(z)
    assert isinstance(q.mag_range, tuple) and all(type(v) is float for v in q.mag_range)
    assert q.mag_range == tuple(float(v) for v in g[f"range.{c}"])
    assert bits_equal(mag_q, g[f"mag_q.{c}"]) and bits_equal(phase_q, g[f"phase_q.{c}"])
    deq = q.dequantize(mag_q, phase_q)
    if f"deq.{c}" in g:
        assert bits_equal(deq, g[f"deq.{c}"])
    assert (torch.norm(deq - z) / torch.norm(z)).item() == float(g[f"rt_err.{c}"])
    assert float(g[f"ref_worst.{c}"]) <= qc.BAND / 10 and float(g[f"deq_err.{c}"]) <= TOL_ACT / 10
    # the range sticks: another tensor is coded with the first one's
    first = q.mag_range
    m2, _ = q.quantize(z * 64)
    assert q.mag_range == first and int(m2.max()) == 2 ** config[0] - 1
    assert bits_equal(m2, fn.polar_quantize(z * 64, *config, first)[0])


def test_polar_range_on_the_cpu_is_the_reference_s_pair():
    z = qc.polar_input((3, 1000))
    r = fn.polar_range(z)
    lg = torch.log2(torch.abs(z).clamp(min=1e-9))
    assert r.dtype == torch.float32 and r.tolist() == [lg.min().item(), lg.max().item()]
    want = qc.polar_range_def(z)
    assert all(abs(a - b) <= 4 * qc.ulp32(max(abs(want[0]), abs(want[1]))) for a, b in zip(r.tolist(), want))
    with pytest.raises(ValueError):
        fn.polar_range(z[:0])
    with pytest.raises(ValueError):
        fn.polar_range(z, max_workgroups=-1)


def test_constant_magnitude_codes_are_zero():
    z = qc.constant_magnitude()
    q = pkg.PolarQuantizer(4, 8)
    mag_q, _ = q.quantize(z)
    assert q.mag_range[0] == q.mag_range[1] and int(mag_q.max()) == 0


def test_log8_gives_the_reference_s_bits():
    g = tensors("R21_log8")
    x = qc.log8_input((3, 1000))
    assert bits_equal(x, g["x"])
    assert bits_equal(Q.log8_encode(x), g["enc"])
    assert bits_equal(Q.log8_decode(torch.arange(256, dtype=torch.uint8)), g["dec"])
    assert float(g["ref_worst"]) <= qc.BAND / 10 and float(g["dec_err"]) <= TOL_ACT / 10
    sp = torch.tensor([0.0, -0.0, 1e-30, 1e30, -1e30])
    assert Q.log8_encode(sp).tolist() == [128, 128, 128, 255, 127]
    re_q, im_q = Q.compress_sparse_freq(g["c.z"], g["c.indices"])
    assert bits_equal(re_q, g["c.re_q"]) and bits_equal(im_q, g["c.im_q"])
    assert bits_equal(Q.decompress_sparse_freq(re_q, im_q, g["c.indices"], (64,)), g["c.out"])
    assert bits_equal(fn.log8_decode_complex(re_q, im_q), torch.complex(Q.log8_decode(re_q), Q.log8_decode(im_q)))


def test_float64_definitions_agree_with_the_reference_s_codes():
    """the yardsticks of the GPU tests, held against the recorded codes with a tenth of the band"""
    z = qc.polar_input((3, 1000))
    g = tensors(qc.polar_name((3, 1000)))
    for mb, pb in [c for c in qc.POLAR_CONFIGS if c[1] <= 8]:
        u, v = qc.polar_uv_def(z, mb, pb, g[f"range.{mb}_{pb}"])
        assert max(qc.band_share(u, "round"), qc.band_share(v, "round")) <= qc.BAND_SHARE
        qc.check_codes(g[f"mag_q.{mb}_{pb}"], u, 2 ** mb - 1, "round", qc.BAND / 10)
        qc.check_codes(g[f"phase_q.{mb}_{pb}"], v, 2 ** pb - 1, "round", qc.BAND / 10)
    with pytest.raises(AssertionError):
        qc.check_codes(g["mag_q.4_8"] + 1, qc.polar_uv_def(z, 4, 8, g["range.4_8"])[0], 15, "round")


# ---- the layer ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", qc.LAYER_SEEDS)
@pytest.mark.parametrize("learn_phase", (True, False))
def test_layer_state_and_forward(rec, seed, learn_phase):
    p = f"layer.{seed}.{int(learn_phase)}"
    torch.manual_seed(seed)
    layer = pkg.FrequencyLinearLayer(qc.LAYER_ARGS[0], qc.LAYER_ARGS[1], sparsity=qc.LAYER_ARGS[2], learn_phase=learn_phase)
    ref_state = {k[len(p) + 7:]: v for k, v in rec.items() if k.startswith(p + ".state.")}
    state = layer.state_dict()
    assert list(state) == list(ref_state) == (["weight_freq", "bias"] if learn_phase else ["weight_magnitude", "bias", "weight_phase"])
    for k, v in ref_state.items():
        assert bits_equal(state[k], v), k
    fresh = pkg.FrequencyLinearLayer(128, 128, sparsity=0.5, learn_phase=learn_phase)
    fresh.load_state_dict(ref_state, strict=True)
    close(p, fresh(rec[p + ".x"]), rec[p + ".out"])
    if learn_phase:
        assert layer.compress_ratio() == float(rec[p + ".ratio"])
    else:
        with pytest.raises(AttributeError):
            layer.compress_ratio()


def test_layer_quirks_are_the_reference_s():
    with pytest.raises(AssertionError):
        pkg.FrequencyLinearLayer(128, 64, sparsity=0.1)(torch.randn(1, 2, 128))
    small = pkg.FrequencyLinearLayer(64, 64)                      # int(64 * 0.01) == 0 kept bins
    assert int(torch.count_nonzero(small.weight_freq)) == 0
    assert pkg.FrequencyLinearLayer(8, 8, bias=False).bias is None


# ---- the transform-based ops ----------------------------------------------------------------------------------------------------

def test_frequency_linear(rec):
    x, w, b = qc.linear_inputs(*qc.LINEAR)
    assert bits_equal(x, rec["linear.x"]) and bits_equal(w, rec["linear.w"])
    close("linear", C.frequency_linear(x, w, b), rec["linear.out"])
    close("linear (function)", pkg.frequency_linear(x, w, b), rec["linear.out"])
    close("linear batched", C.frequency_linear_batched(x, w, b, chunk_size=1), rec["linear.batched"])
    assert rel_err(C.frequency_linear(x, w, b).numpy(), qc.linear_def(x, w, b).numpy()) <= TOL_ACT
    xc, w, b = qc.linear_inputs(2, 3, 16, 16, complex_x=True)
    assert rel_err(C.frequency_linear(xc, w, b).numpy(), qc.linear_def(xc, w, b).numpy()) <= TOL_ACT


@pytest.mark.parametrize("i", range(len(qc.CONV1D)))
def test_frequency_conv1d(rec, i):
    case = qc.CONV1D[i]
    x, w = qc.conv1d_inputs(case)
    assert bits_equal(x, rec[f"conv1d.{i}.x"]) and bits_equal(w, rec[f"conv1d.{i}.w"])
    out = C.frequency_conv1d(x, w, stride=case[6], padding=case[5])
    close(f"conv1d {case}", out, rec[f"conv1d.{i}.out"])
    close(f"conv1d {case} (function)", pkg.frequency_conv1d(x, w, case[6], case[5]), rec[f"conv1d.{i}.out"])
    assert rel_err(out.numpy(), qc.conv_def(x, w, case[6], case[5]).numpy()) <= TOL_ACT


def test_frequency_conv2d_and_conv3d(rec):
    x, w = qc.conv2d_inputs()
    out = C.frequency_conv2d(x, w, stride=qc.CONV2D[8], padding=qc.CONV2D[7])
    close("conv2d", out, rec["conv2d.out"])
    assert rel_err(out.numpy(), qc.conv_def(x, w, qc.CONV2D[8], qc.CONV2D[7]).numpy()) <= TOL_ACT
    x, w = qc.conv3d_inputs()
    out = C.frequency_conv3d(x, w)
    close("conv3d", out, rec["conv3d.out"])
    assert rel_err(out.numpy(), qc.conv_def(x, w, 1, 0).numpy()) <= TOL_ACT


def test_wirtinger_autograd(rec):
    x = rec["wirtinger.x"].clone().requires_grad_(True)
    w = rec["wirtinger.w"].clone().requires_grad_(True)
    y = pkg.WirtingerAutograd.apply(x, w)
    y.backward(rec["wirtinger.g"])
    assert bits_equal(y.detach(), rec["wirtinger.out"])
    assert bits_equal(x.grad, rec["wirtinger.grad_x"]) and bits_equal(w.grad, rec["wirtinger.grad_w"])


def test_gradcheck_of_the_cpu_path():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 6, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.complex(torch.randn(6, 4, generator=g, dtype=torch.float64),
                      torch.randn(6, 4, generator=g, dtype=torch.float64)).requires_grad_(True)
    b = torch.randn(4, generator=g, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(C.frequency_linear, (x, w, b))
    x = torch.randn(2, 2, 9, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.complex(torch.randn(3, 2, 4, generator=g, dtype=torch.float64),
                      torch.randn(3, 2, 4, generator=g, dtype=torch.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, c: C.frequency_conv1d(a, c, 2, 1), (x, w))


# ---- the converter --------------------------------------------------------------------------------------------------------------

def _linear(rec):
    lin = torch.nn.Linear(128, 128)
    with torch.no_grad():
        lin.weight.copy_(rec["convert.weight"])
        lin.bias.copy_(rec["convert.bias"])
    return lin


@pytest.mark.parametrize("learn_phase", (True, False))
def test_converted_linear_equals_the_reference_s(rec, learn_phase):
    conv = pkg.FFTConverter.convert_linear_to_frequency(_linear(rec), sparsity=0.1, learn_phase=learn_phase, quantize=True)
    assert isinstance(conv, pkg.FrequencyLinearLayer)
    ref_state = {k[len("convert.0."):]: v for k, v in rec.items() if k.startswith(f"convert.{int(learn_phase)}.")}
    assert list(conv.state_dict()) == list(ref_state)
    for k, v in ref_state.items():
        assert bits_equal(conv.state_dict()[k], v), k


def test_convert_model_and_save(rec, tmp_path):
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embed_proj = torch.nn.Linear(128, 128)
            self.body = torch.nn.Sequential(torch.nn.Linear(128, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128, bias=False))
            self.head = torch.nn.Linear(128, 128)
            self.lm_head = torch.nn.Linear(128, 128)
    net = Net()
    assert pkg.FFTConverter.convert_model(net, sparsity=0.1) is net
    for m in (net.embed_proj, net.head, net.lm_head, net.body[1]):
        assert not isinstance(m, pkg.FrequencyLinearLayer)
    assert isinstance(net.body[0], pkg.FrequencyLinearLayer) and isinstance(net.body[2], pkg.FrequencyLinearLayer)
    assert net.body[2].bias is None
    pkg.FFTConverter.save_fft_model(net, str(tmp_path / "m"))
    assert sorted(os.listdir(tmp_path / "m")) == ["config.json", "weights.fft"]
    cfg = json.load(open(tmp_path / "m" / "config.json"))
    assert sorted(cfg) == ["compression", "num_layers"] and cfg["num_layers"] == 2
    layers = torch.load(tmp_path / "m" / "weights.fft", weights_only=False)
    assert sorted(layers) == ["body.0", "body.2"]
    assert sorted(layers["body.0"]) == ["bias", "in_features", "out_features", "sparsity", "weight_freq"]
    assert layers["body.2"]["bias"] is None and bits_equal(layers["body.0"]["weight_freq"], net.body[0].weight_freq.data)
    assert cfg["compression"] == pytest.approx(128 * 128 / (128 * 12), rel=1e-12)
