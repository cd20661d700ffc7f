"""The dual head without a GPU: exports and state_dict keys, the torch fallback of functional.cross_entropy against
F.cross_entropy bit for bit, get_token_ids_fast against the reference's vectors (K22), DualHead / compute_dual_loss on
the CPU against K21, and the ABI surface of the smx_xent_* entries (every refusal comes before any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dual_common as dc
import heads_common as hc
from conftest import ROOT, TOL_ACT, TOL_PARAM, load_golden, rel_err

HDR = os.path.join(ROOT, "include", "smx.h")
ENTRIES = ("smx_xent_supported", "smx_xent_workspace_bytes", "smx_xent_forward", "smx_xent_backward")
NAMES = ("DualHead", "TokenAwareChunkLM", "get_token_ids_fast", "compute_dual_loss", "get_gpt2_tokenizer", "cross_entropy")


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
    z = load_golden("K22_token_ids")
    m = pkg.TokenAwareChunkLM(hc.StubBackbone(8), 4)
    assert sorted(m.state_dict()) == list(z["keys"])
    assert {"head.char_head.weight", "head.char_head.bias", "head.token_head.weight", "head.token_head.bias"} <= set(z["keys"])
    assert m.chunk == 4 and m.tokenizer is None and pkg.TokenAwareChunkLM(hc.StubBackbone(8), 2, tokenizer="t").tokenizer == "t"
    assert m.head.char_head.weight.shape == (256, 8) and m.head.token_head.weight.shape == (50257, 8)
    h = pkg.DualHead(16, token_vocab_size=300)
    assert (h.d_model, h.vocab_size, h.token_vocab_size) == (16, 256, 300)
    for lin in (h.char_head, h.token_head):
        assert not lin.bias.any() and 0.015 < float(lin.weight.detach().std()) < 0.025
    assert pkg.DualHead(4, 7, 9).char_head.weight.shape == (7, 4)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("ignore_index", [-100, 0, 3])
def test_cpu_fallback_is_torch_cross_entropy_bit_for_bit(reduction, ignore_index):
    import tensor_cuda_fft_amd as pkg
    torch.manual_seed(3)
    x = (3.0 * torch.randn(4, 5, 19)).requires_grad_(True)
    y = torch.randint(0, 19, (4, 5))
    y[0, :2] = 3
    y[2, 1] = 0
    x2 = x.detach().clone().requires_grad_(True)
    got = pkg.cross_entropy(x, y, ignore_index=ignore_index, reduction=reduction)
    ref = torch.nn.functional.cross_entropy(x2.reshape(-1, 19), y.reshape(-1), ignore_index=ignore_index,
                                            reduction=reduction)
    assert type(got.grad_fn).__name__.find("_CrossEntropy") < 0
    assert got.shape == (y.shape if reduction == "none" else ())
    assert torch.equal(got.reshape(-1), ref.reshape(-1))
    g = torch.randn_like(got)
    got.backward(g)
    ref.backward(g.reshape(ref.shape))
    assert torch.equal(x.grad, x2.grad)


def test_cross_entropy_argument_checks_and_defaults():
    import tensor_cuda_fft_amd as pkg
    x, y = torch.randn(6, 11), torch.randint(0, 11, (6,))
    y[1] = -100
    assert torch.equal(pkg.cross_entropy(x, y), torch.nn.functional.cross_entropy(x, y))          # ignore_index = -100, mean
    with pytest.raises(ValueError, match="reduction"):
        pkg.cross_entropy(x, y, reduction="batchmean")
    with pytest.raises(ValueError, match="targets of shape"):
        pkg.cross_entropy(x, y[:5])
    assert pkg.cross_entropy(torch.zeros(0, 11), torch.zeros(0, dtype=torch.int64), reduction="none").shape == (0,)
    assert torch.equal(pkg.cross_entropy(x[0], y[0]), torch.nn.functional.cross_entropy(x[:1], y[:1]))   # (V) and ()


@pytest.mark.parametrize("key", ["text", "invalid_utf8", "blank", "one_token", "many_tokens", "raising"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_token_ids_reproduce_the_reference(key, dtype):
    import tensor_cuda_fft_amd as pkg
    z = load_golden("K22_token_ids")
    rows = dc.token_id_rows()
    tok, x = rows[key]
    assert np.array_equal(x, z[key + ".x"]) and str(z[key + ".tokenizer"]) == tok          # the fixture is of these rows
    ids = pkg.get_token_ids_fast(hc.t(x).to(dtype), dc.TOKENIZERS[tok]())
    assert ids.dtype == dtype and ids.device.type == "cpu" and ids.shape == x.shape
    assert np.array_equal(ids.numpy(), z[key + ".ids"])
    if key == "many_tokens":                                                                  # n > T: c = 0
        assert (ids == ids[:, -1:]).all() and ids.all()
    if key == "blank":
        assert not ids[:2].any() and ids[2].all()


def test_token_ids_closed_form_on_other_widths():
    import tensor_cuda_fft_amd as pkg
    g = np.random.default_rng(5)
    for T in (1, 7, 33):
        x = hc.t(g.choice(np.array([32, 32, 97, 98, 99, 100]), (5, T)).astype(np.int64))
        assert torch.equal(pkg.get_token_ids_fast(x, dc.StubTokenizer()), dc.stub_token_targets(x)), T
    assert pkg.get_token_ids_fast(torch.zeros((0, 4), dtype=torch.int64), dc.StubTokenizer()).shape == (0, 4)


def test_dual_head_and_loss_on_the_cpu_match_the_reference():
    import tensor_cuda_fft_amd as pkg
    z = load_golden("K21_dual_loss")
    assert (z["y_token"] == 0).sum() >= 5 and float(z["ref_err_token_logits"]) <= TOL_ACT / 4
    got, _ = dc.run_k21(pkg, z)
    dc.check_k21(got, z)
    head = dc.load_head(pkg, z)
    only = head(hc.t(z["hidden"]), return_token_logits=False)
    assert isinstance(only, torch.Tensor) and torch.equal(only, got["char_logits"])


def test_loss_defaults_are_the_reference_weights():
    import tensor_cuda_fft_amd as pkg
    torch.manual_seed(0)
    cl, tl = torch.randn(2, 4, 256), torch.randn(2, 9, 40)
    yc, yt = torch.randint(0, 256, (2, 4)), torch.randint(0, 40, (2, 9))
    yt[0, :3] = 0
    total, c, t = pkg.compute_dual_loss(cl, tl, yc, yt)
    assert torch.equal(c, torch.nn.functional.cross_entropy(cl.reshape(-1, 256), yc.reshape(-1)))
    assert torch.equal(t, torch.nn.functional.cross_entropy(tl.reshape(-1, 40), yt.reshape(-1), ignore_index=0))
    assert torch.allclose(total, c + 0.5 * t)
    assert torch.allclose(pkg.compute_dual_loss(cl, tl, yc, yt, 2.0, 0.25)[0], 2.0 * c + 0.25 * t)


def test_token_aware_model_shapes_in_train_and_eval():
    import tensor_cuda_fft_amd as pkg
    torch.manual_seed(1)
    m = pkg.TokenAwareChunkLM(hc.StubBackbone(8), 4)
    x = torch.randint(0, 256, (2, 12))
    m.train()
    char_logits, token_logits = m(x)
    assert char_logits.shape == (2, 4, 256) and token_logits.shape == (2, 12, 50257)
    full = m.head(m.backbone.last_hidden)[0][:, -4:, :]                    # the reference's order: all rows, then the slice
    assert rel_err(char_logits.detach().numpy(), full.detach().numpy()) <= TOL_ACT
    only = m(x, return_token_logits=False)
    assert isinstance(only, torch.Tensor) and only.shape == (2, 4, 256)
    m.eval()
    with torch.no_grad():
        assert isinstance(m(x), torch.Tensor) and m(x).shape == (2, 4, 256)
        both = m(x, return_token_logits=True)
        assert isinstance(both, tuple) and both[1].shape == (2, 12, 50257)


def test_header_declares_and_cites_the_xent_entries():
    src = open(HDR).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
    assert "fft_lm/dual_head.py:176-188" in src and "DIFFERENCE FROM TORCH" in src
    assert re.search(r"#define SMX_VERSION 303\b", src)
    assert [int(re.search(r"#define SMX_XENT_%s (\d)" % n, src).group(1)) for n in ("MEAN", "SUM", "NONE")] == [0, 1, 2]


def test_binding_covers_the_xent_entries_and_the_version_stays(L):
    assert set(ENTRIES) <= set(L._SIGS)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert L.lib().smx_version() == 303


def test_xent_argument_validation_without_a_device(L):
    lib = L.lib()
    err = lambda: lib.smx_last_error().decode()
    buf = (ctypes.c_float * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255                                      # 256-byte aligned host memory
    INVALID, WORKSPACE = -1, -4
    n = ctypes.c_size_t()
    assert [lib.smx_xent_supported(v) for v in (1, 6, 256, 4099, 50257, 2 ** 31 - 1)] == [1] * 6
    assert [lib.smx_xent_supported(v) for v in (0, -1)] == [0, 0]
    sizes = []
    for R, V in ((1, 256), (37, 6), (8192, 50257), (8192, 256), (1 << 20, 4099)):
        assert lib.smx_xent_workspace_bytes(R, V, ctypes.byref(n)) == 0
        assert n.value % 256 == 0 and n.value >= 65536 + 8 * min(R, 2048)          # one (sum, count) pair per workgroup
        sizes.append(n.value)
    assert sizes[2] == sizes[3] == sizes[4] and sizes[0] < sizes[2]
    assert lib.smx_xent_workspace_bytes(4, 8, None) == INVALID
    assert lib.smx_xent_workspace_bytes(0, 8, ctypes.byref(n)) == INVALID and "positive" in err()
    assert lib.smx_xent_workspace_bytes(4, 0, ctypes.byref(n)) == INVALID and "positive" in err()
    assert lib.smx_xent_workspace_bytes(1 << 31, 8, ctypes.byref(n)) == INVALID and "too large" in err()
    fw, bw = lib.smx_xent_forward, lib.smx_xent_backward
    ws, wsn = p + 8192, 1 << 17
    ok = dict(x=p, st=8, t=p + 1024, ig=-100, red=0, loss=p + 2048, lse=p + 2304, cnt=p + 2560)

    def f(ws_=ws, wsn_=wsn, R=4, V=8, **kw):
        a = dict(ok, **kw)
        return fw(a["x"], a["st"], a["t"], a["ig"], a["red"], a["loss"], a["lse"], a["cnt"], ws_, wsn_, R, V, None)

    for name in ("x", "t", "loss", "lse", "cnt"):
        assert f(**{name: None}) == INVALID and "non-NULL" in err(), name
    assert f(R=0) == INVALID and "positive" in err()
    assert f(R=-2) == INVALID
    assert f(V=0) == INVALID and "positive" in err()
    assert f(st=7) == INVALID and "row_stride" in err()
    for bad in (-1, 3, 99):
        assert f(red=bad) == INVALID and "reduction" in err()
    assert f(x=p + 2) == INVALID and "aligned" in err()
    assert f(t=p + 1028) == INVALID and "8-byte" in err()
    assert f(ws_=None, wsn_=0) == WORKSPACE and "smx_xent_workspace_bytes" in err()
    assert f(wsn_=1024) == WORKSPACE
    assert f(ws_=ws + 8) in (WORKSPACE, INVALID) and "aligned" in err()

    def b(R=4, V=8, **kw):
        a = dict(dict(ok, g=p + 3072, grad=p + 4096), **kw)
        return bw(a["g"], a["x"], a["st"], a["t"], a["ig"], a["red"], a["lse"], a["cnt"], a["grad"], R, V, None)

    for name in ("g", "x", "t", "lse", "cnt", "grad"):
        assert b(**{name: None}) == INVALID and "non-NULL" in err(), name
    assert b(R=0) == INVALID and "positive" in err()
    assert b(V=-1) == INVALID
    assert b(st=3) == INVALID and "row_stride" in err()
    assert b(red=3) == INVALID and "reduction" in err()
    assert b(grad=p + 4098) == INVALID and "aligned" in err()
    assert b(grad=p) == INVALID and "alias" in err()
