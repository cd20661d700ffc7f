"""The word-structure heads without a GPU: exports and state_dict keys, the torch path of the two target functions against
the reference's golden vectors (K01) and the fp64 closed form, losses and model forward / backward on the CPU fallback
against K11 / K12, and the ABI surface of the new entries (every refusal comes before any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import heads_common as hc
from conftest import ROOT, TOL_ACT, TOL_PARAM, load_golden, rel_err

HDR = os.path.join(ROOT, "include", "smx.h")
ENTRIES = ("smx_word_targets", "smx_head_supported", "smx_head_workspace_bytes", "smx_head_forward", "smx_head_backward")
NAMES = ("PhaseClockHead", "PhaseClockChunkLM", "generate_phase_targets", "compute_phase_clock_loss", "SegmentationHead",
         "SegmentedChunkLM", "get_word_boundaries", "compute_segmented_loss", "word_targets", "narrow_head")
MODELS = {"K11_phaseclock_2x48x32": ("PhaseClockChunkLM", "compute_phase_clock_loss", "generate_phase_targets", "phase_head"),
          "K12_segmented_2x48x32": ("SegmentedChunkLM", "compute_segmented_loss", "get_word_boundaries", "seg_head")}


@pytest.fixture(scope="module")
def L():
    import subprocess
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


def test_exports_constructors_and_state_dict_keys():
    import tensor_cuda_fft_amd as pkg
    for name in NAMES:
        assert name in pkg.__all__ and hasattr(pkg, name), name
    for gname, (cls, _, _, head) in MODELS.items():
        z = load_golden(gname)
        m = getattr(pkg, cls)(hc.StubBackbone(int(z["d_model"])), int(z["chunk"]))
        assert sorted(m.state_dict()) == list(z["keys"])
        assert m.chunk == int(z["chunk"]) and m.char_head.weight.shape == (256, 32)
        hd = getattr(m, head).head
        assert not hd.weight.any() and not hd.bias.any()                          # the heads start at zero
        assert not m.char_head.bias.any() and 0.01 < float(m.char_head.weight.detach().std()) < 0.03
        m.load_state_dict({k[3:]: hc.t(v) for k, v in z.items() if k.startswith("sd.")}, strict=True)
    assert pkg.PhaseClockHead(8).head.weight.shape == (2, 8) and pkg.SegmentationHead(8).head.weight.shape == (1, 8)
    keys = set(pkg.PhaseClockChunkLM(hc.StubBackbone(8), 2).state_dict())
    assert {"char_head.weight", "char_head.bias", "phase_head.head.weight", "phase_head.head.bias"} <= keys
    assert {"seg_head.head.weight", "seg_head.head.bias"} <= set(pkg.SegmentedChunkLM(hc.StubBackbone(8), 2).state_dict())


@pytest.mark.parametrize("key", ["text", "random", "edge"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
def test_cpu_targets_match_the_reference_and_the_closed_form(key, dtype):
    import tensor_cuda_fft_amd as pkg
    z = load_golden("K01_word_targets")
    x = hc.t(z[key + ".x"]).to(dtype)
    assert float(z[key + ".ref_err_phase"]) <= TOL_ACT / 4
    ph, bd = pkg.word_targets(x)
    assert ph.dtype == torch.float32 and bd.dtype == torch.float32 and ph.shape == x.shape + (2,) and bd.shape == x.shape
    assert np.array_equal(bd.numpy(), z[key + ".boundary"])
    assert np.array_equal(bd.numpy(), hc.boundary_closed_form(z[key + ".x"]))
    assert rel_err(ph.numpy(), z[key + ".phase"]) <= TOL_ACT
    assert rel_err(ph.numpy(), hc.phase_closed_form(z[key + ".x"])) <= TOL_ACT
    assert torch.equal(pkg.generate_phase_targets(x), ph) and torch.equal(pkg.get_word_boundaries(x), bd)
    assert pkg.word_targets(x, boundary=False)[1] is None and pkg.word_targets(x, phase=False)[0] is None


@pytest.mark.parametrize("T", [1, 2, 65, 257])
def test_cpu_targets_on_every_pattern(T):
    import tensor_cuda_fft_amd as pkg
    cases = dict(hc.patterns(3, T))
    cases["wide_values"] = hc.wide_values(3, T)
    for name, x in cases.items():
        ph, bd = pkg.word_targets(hc.t(x))
        ref = hc.phase_closed_form(x)
        assert np.array_equal(bd.numpy(), hc.boundary_closed_form(x)), name
        assert rel_err(ph.numpy(), ref) <= TOL_ACT, name
        exact = (ref == 0).all(-1) | ((ref[..., 0] == 1) & (ref[..., 1] == 0))    # delimiters and word starts
        assert np.array_equal(ph.numpy()[exact], ref[exact].astype(np.float32)), name


def test_word_targets_argument_checks():
    import tensor_cuda_fft_amd as pkg
    with pytest.raises(TypeError):
        pkg.word_targets(torch.zeros(2, 3))
    with pytest.raises(TypeError):
        pkg.word_targets(torch.zeros(6, dtype=torch.uint8))
    with pytest.raises(ValueError):
        pkg.word_targets(torch.zeros(2, 3, dtype=torch.uint8), phase=False, boundary=False)
    ph, bd = pkg.word_targets(torch.zeros(0, 5, dtype=torch.int64))
    assert ph.shape == (0, 5, 2) and bd.shape == (0, 5)


@pytest.mark.parametrize("gname", sorted(MODELS))
def test_models_and_losses_on_the_cpu_fallback_match_the_reference(gname):
    import tensor_cuda_fft_amd as pkg
    cls, loss_fn, target_fn, head = MODELS[gname]
    z = load_golden(gname)
    m = getattr(pkg, cls)(hc.StubBackbone(int(z["d_model"])), int(z["chunk"]))
    m.load_state_dict({k[3:]: hc.t(v) for k, v in z.items() if k.startswith("sd.")}, strict=True)
    x = hc.t(z["x"])
    aux_t = getattr(pkg, target_fn)(x)
    assert rel_err(aux_t.numpy(), z["aux_targets"]) <= TOL_ACT
    m.train()
    logits, aux = m(x)                                                            # training mode: both outputs
    total, char_l, aux_l = getattr(pkg, loss_fn)(logits, aux, hc.t(z["y_char"]), aux_t)
    total.backward()
    got = {"char_logits": logits, "aux": aux, "loss_total": total, "loss_char": char_l, "loss_aux": aux_l,
           "grad.hidden": m.backbone.last_hidden.grad}
    got.update({"grad." + k: p.grad for k, p in m.named_parameters() if not k.startswith("backbone.")})
    for k, v in got.items():
        tol = TOL_PARAM if k.startswith("grad.") and k != "grad.hidden" else TOL_ACT
        assert float(z["ref_err_" + k]) <= tol / 4
        assert rel_err(v.detach().numpy(), z[k]) <= tol, k
    assert aux.shape == ((2, 48, 2) if head == "phase_head" else (2, 48))
    m.eval()
    with torch.no_grad():
        only = m(x)
        assert isinstance(only, torch.Tensor) and only.shape == (2, int(z["chunk"]), 256)   # eval: char logits only
        both = m(x, **{"return_phase_vectors" if head == "phase_head" else "return_seg_logits": True})
        assert isinstance(both, tuple) and torch.equal(both[0], only)


def test_loss_defaults_are_the_reference_weights():
    import tensor_cuda_fft_amd as pkg
    torch.manual_seed(0)
    logits, y = torch.randn(2, 4, 256), torch.randint(0, 256, (2, 4))
    pv, pt = torch.randn(2, 9, 2), torch.randn(2, 9, 2)
    total, c, p = pkg.compute_phase_clock_loss(logits, pv, y, pt)
    assert torch.allclose(total, c + 5.0 * p) and torch.allclose(p, ((pv - pt) ** 2).mean())
    sl, st = torch.randn(2, 9), torch.randint(0, 2, (2, 9)).float()
    total, c, s = pkg.compute_segmented_loss(logits, sl, y, st)
    assert torch.allclose(total, c + 0.1 * s)
    assert torch.allclose(pkg.compute_segmented_loss(logits, sl, y, st, 2.0, 0.5)[0], 2.0 * c + 0.5 * s)


def test_narrow_head_on_the_cpu_is_linear():
    import tensor_cuda_fft_amd as pkg
    torch.manual_seed(1)
    h, w, b = torch.randn(3, 5, 12, requires_grad=True), torch.randn(2, 12, requires_grad=True), torch.randn(2)
    y = pkg.narrow_head(h, w, b)
    assert torch.equal(y, torch.nn.functional.linear(h, w, b))
    y.sum().backward()
    assert h.grad is not None and w.grad is not None
    assert pkg.narrow_head(h.detach(), w[:1].detach()).shape == (3, 5, 1)


def test_header_declares_and_cites_the_head_entries():
    src = open(HDR).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
    for cite in ("fft_lm/phase_clock.py:83-113", "fft_lm/segmentation_head.py:77-97", "fft_lm/phase_clock.py:53,65",
                 "fft_lm/segmentation_head.py:43,55"):
        assert cite in src
    assert re.search(r"#define SMX_VERSION 303\b", src)


def test_binding_covers_the_head_entries_and_the_version_stays(L):
    assert set(ENTRIES) <= set(L._SIGS)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert L.lib().smx_version() == 303


def test_argument_validation_without_a_device(L):
    lib = L.lib()
    err = lambda: lib.smx_last_error().decode()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255                                      # 256-byte aligned host memory
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    wt = lib.smx_word_targets
    assert wt(None, 1, 64, p, p, 2, 64, None) == INVALID and "tokens" in err()
    assert wt(p, 1, 64, None, None, 2, 64, None) == INVALID and "both NULL" in err()
    for bad in (0, 2, 4, 16):
        assert wt(p, bad, 64, p, p, 2, 64, None) == INVALID and "token_bytes" in err()
    assert wt(p + 4, 8, 64, p, p, 2, 64, None) == INVALID and "8-byte aligned" in err()
    assert wt(p, 1, 63, p, p, 2, 64, None) == INVALID and "row_stride" in err()
    assert wt(p, 1, 64, p, p, 0, 64, None) == INVALID and "positive" in err()
    assert wt(p, 1, 64, p, p, -1, 64, None) == INVALID
    assert wt(p, 1, 64, p, p, 2, 0, None) == INVALID and "positive" in err()
    assert wt(p, 1, 65537, p, p, 2, 65537, None) == INVALID and "at most 65536" in err()
    assert wt(p, 1, 65536, p, p, 32768, 65536, None) == INVALID and "too large" in err()
    assert wt(p, 1, 64, p + 4, None, 2, 64, None) == INVALID and "aligned" in err()
    # the head: shape, O, C, pointers, workspace
    n = ctypes.c_size_t()
    assert [lib.smx_head_supported(c, o) for c, o in ((512, 1), (512, 2), (6, 2), (4096, 1), (1024, 2), (1023, 1))] == [1] * 6
    assert [lib.smx_head_supported(c, o) for c, o in ((512, 0), (512, 3), (0, 1), (4100, 1), (1025, 2), (-4, 1))] == [0] * 6
    assert lib.smx_head_workspace_bytes(8192, 512, 2, ctypes.byref(n)) == 0
    assert n.value >= 2048 * 2 * 512 * 4 + 2048 * 2 * 4 and n.value % 256 == 0    # grad_w and grad_b partials of 2048 blocks
    big = n.value
    assert lib.smx_head_workspace_bytes(37, 512, 1, ctypes.byref(n)) == 0 and n.value < big
    assert lib.smx_head_workspace_bytes(37, 512, 1, None) == INVALID
    assert lib.smx_head_workspace_bytes(0, 512, 1, ctypes.byref(n)) == INVALID and "positive" in err()
    assert lib.smx_head_workspace_bytes(37, 512, 3, ctypes.byref(n)) == UNSUPPORTED and "O = 1 or 2" in err()
    assert lib.smx_head_workspace_bytes(37, 1025, 1, ctypes.byref(n)) == UNSUPPORTED and "not supported" in err()
    fw, bw = lib.smx_head_forward, lib.smx_head_backward
    assert fw(None, p, p, p, 4, 8, 2, None) == INVALID and "non-NULL" in err()
    assert fw(p, None, p, p, 4, 8, 2, None) == INVALID
    assert fw(p, p, p, None, 4, 8, 2, None) == INVALID
    assert fw(p, p, None, p, 0, 8, 2, None) == INVALID and "positive" in err()
    assert fw(p, p, None, p, -3, 8, 2, None) == INVALID
    assert fw(p, p, None, p, 4, 8, 0, None) == UNSUPPORTED
    assert fw(p, p, None, p, 4, 4100, 1, None) == UNSUPPORTED
    assert fw(p + 4, p, None, p, 4, 8, 1, None) == INVALID and "16-byte" in err()
    ws, wsn = p + 4096, 1 << 20
    assert bw(None, p, p, p, p, p, ws, wsn, 4, 8, 2, None) == INVALID and "non-NULL" in err()
    assert bw(p, None, p, p, p, p, ws, wsn, 4, 8, 2, None) == INVALID             # grad_w needs h
    assert bw(p, p, None, p, p, p, ws, wsn, 4, 8, 2, None) == INVALID             # grad_h needs w
    assert bw(p, p, p, p, p, p, ws, wsn, 4, 8, 3, None) == UNSUPPORTED
    assert bw(p, p, p, p, p, p, ws, wsn, 4, 1026, 2, None) == UNSUPPORTED
    assert bw(p, p, p, p, p, p, ws, wsn, 0, 8, 2, None) == INVALID
    assert bw(p, p, p, p + 256, p, p, None, 0, 4, 8, 2, None) == WORKSPACE and "smx_head_workspace_bytes" in err()
    assert bw(p, p, p, p + 256, p, p, ws, 1024, 4, 8, 2, None) == WORKSPACE
    assert bw(p, p, p, p + 256, p, p, ws + 8, wsn, 4, 8, 2, None) in (WORKSPACE, INVALID) and "aligned" in err()
    assert bw(p, p, p, p, p, p, ws, wsn, 4, 8, 2, None) == INVALID and "alias" in err()
