"""The byte-spectral models without a GPU: the torch path of functional.byte_features (what CPU tokens run) against the
float64 table of tests/byte_common.py and the reference's recorded vectors Z01-Z21, the modules' state_dict layout, the
ABI surface of the smx_byte_* entries, the band gradient, the edge rows, and generation's stop rule.

Tolerance of the feature rows: TOL_FACTOR * r_ref, r_ref being the reference's own largest normalised error against the
table over the fixtures (measured: r_ref = 1.67e-07; the torch path, a float64 FFT rounded once, 6.5e-08 at worst)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import byte_common as bc
from conftest import ROOT, TOL_ACT, TOL_PARAM, load_golden, rel_err

HDR = os.path.join(ROOT, "include", "smx.h")
ENTRIES = ("smx_byte_supported", "smx_byte_features", "smx_byte_workspace_bytes", "smx_byte_grad_bands")
NAMES = ("ByteSpectralEmbedding", "ByteSpectralEncoder", "SpectralLanguageModel", "byte_features")
SHAPES = [(2, 1, 8), (2, 2, 8), (3, 10, 12), (2, 37, 32), (2, 64, 32), (2, 300, 64), (2, 512, 256), (1, 4096, 8)]


@pytest.fixture(scope="module")
def L():
    import subprocess
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


def pkg():
    import tensor_cuda_fft_amd
    return tensor_cuda_fft_amd


def sd_of(z):
    return {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd.")}


def test_names_are_exported():
    p = pkg()
    for n in NAMES:
        assert n in p.__all__ and hasattr(p, n), n


def test_header_declares_and_cites_the_byte_entries():
    src = open(HDR).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
    for cite in ("byte_spectral_model.py:44-102", "byte_spectral.py:53-108"):
        assert cite in src
    assert re.search(r"#define SMX_VERSION 303\b", src)


def test_binding_covers_the_byte_entries_and_the_version_stays(L):
    assert set(ENTRIES) <= set(L._SIGS)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert L.lib().smx_version() == 303


def test_supported_range_and_refusals_without_a_device(L):
    lib = L.lib()
    err = lambda: lib.smx_last_error().decode()
    sup = lib.smx_byte_supported
    assert [sup(1, 0, 1), sup(4096, 2048, 4096), sup(512, 128, 256), sup(10, 5, 12)] == [1, 1, 1, 1]
    assert [sup(0, 0, 8), sup(4097, 4, 8), sup(64, 33, 64), sup(64, 16, 0), sup(64, 16, 4097), sup(64, -1, 8)] == [0] * 6
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    feat = lib.smx_byte_features
    assert feat(None, 1, 64, p, p, None, 2, 64, 16, 32, 64, None) == INVALID and "non-NULL" in err()
    assert feat(p, 1, 64, p, None, None, 2, 64, 16, 32, 64, None) == INVALID and "non-NULL" in err()
    assert feat(p, 1, 64, None, p, None, 2, 64, 16, 32, 64, None) == INVALID and "bands" in err()
    assert feat(p, 4, 64, p, p, None, 2, 64, 16, 32, 64, None) == INVALID and "token_bytes" in err()
    assert feat(p, 1, 64, p, p, None, 2, 64, 16, 32, 2, None) == INVALID and "P must be 1" in err()
    assert feat(p, 1, 64, p, p, None, 2, 64, 33, 80, 64, None) == INVALID and "T / 2" in err()
    assert feat(p, 1, 10, p, p, None, 2, 64, 16, 32, 64, None) == INVALID and "row_stride" in err()
    assert feat(p, 1, 64, p, p + 4, None, 2, 64, 16, 32, 64, None) == INVALID and "16-byte" in err()
    assert feat(p + 4, 8, 64, p, p, None, 2, 64, 16, 32, 64, None) == INVALID and "8-byte" in err()
    assert feat(p, 1, 64, p, p, None, 0, 64, 16, 32, 64, None) == INVALID and "positive" in err()
    assert feat(p, 1, 8192, p, p, None, 2, 4097, 4, 8, 4097, None) == UNSUPPORTED and "smx_byte_supported" in err()
    assert feat(p, 1, 64, p, p, None, 2, 64, 16, 4100, 64, None) == UNSUPPORTED
    n = ctypes.c_size_t()
    wsb = lib.smx_byte_workspace_bytes
    assert wsb(64, 512, 256, 128, ctypes.byref(n)) == 0 and n.value == 64 * 8 * 128 * 4     # (b, 64 rows) x column
    assert wsb(2, 1, 32, 16, ctypes.byref(n)) == 0 and n.value == 256
    assert wsb(2, 1, 8, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert wsb(2, 64, 32, 16, None) == INVALID and wsb(0, 64, 32, 16, ctypes.byref(n)) == INVALID
    gb = lib.smx_byte_grad_bands
    assert gb(None, p, p, 16, p, 1 << 12, 2, 64, 32, 16, None) == INVALID and "non-NULL" in err()
    assert gb(p, None, p, 16, p, 1 << 12, 2, 64, 32, 16, None) == INVALID
    assert gb(p, p, p, 8, p, 1 << 12, 2, 64, 32, 16, None) == INVALID and "n_bands" in err()
    assert gb(p, p, p, 16, None, 0, 2, 64, 32, 16, None) == WORKSPACE and "smx_byte_workspace_bytes" in err()
    assert gb(p, p, p, 16, p, 64, 2, 64, 32, 16, None) == WORKSPACE
    assert gb(p, p, p, 16, p + 16, 1 << 12, 2, 64, 32, 16, None) == INVALID and "256-byte" in err()


def test_reference_yardstick_is_what_the_docstring_says():
    r = bc.r_ref()
    print(f"r_ref = {r:.3e}")
    assert 1e-8 < r < 1e-6                      # fp32 rounding of an FFT against float64, normalised


@pytest.mark.parametrize("name", bc.EMBEDDING_FIXTURES + bc.ENCODER_FIXTURES + (bc.LM_FIXTURE,))
def test_torch_path_against_the_fixtures(name):
    z = load_golden(name)
    pos = name not in bc.ENCODER_FIXTURES
    W = int(z["width"])
    out = pkg().byte_features(torch.from_numpy(z["ids"]), torch.from_numpy(z["bands"]), W, positions=pos)
    e, share = bc.compare(out.numpy(), z["ids"], z["bands"], W, pos)
    print(f"{name}: torch path {e:.3e}, r_ref {bc.r_ref():.3e}")
    assert share == 0.0 and e <= bc.TOL_FACTOR * bc.r_ref()


@pytest.mark.parametrize("B,T,W", SHAPES)
def test_torch_path_against_the_table(B, T, W):
    g = torch.Generator().manual_seed(B * 100000 + T * 10 + W)
    ids = torch.randint(0, 256, (B, T), generator=g, dtype=torch.int64)
    if T == 2:
        ids[0] = torch.tensor([3, 50])          # a negative DC, a positive one below
        ids[1] = torch.tensor([200, 180])
    bands = torch.rand(W // 2, generator=g) + 0.5
    out = pkg().byte_features(ids, bands, W)
    e, share = bc.compare(out.numpy(), ids.numpy(), bands.numpy(), W)
    print(f"({B}, {T}, {W}): torch path {e:.3e}, left out {share:.2%}")
    assert e <= bc.TOL_FACTOR * bc.r_ref()
    u8 = pkg().byte_features(ids.to(torch.uint8), bands, W)
    assert torch.equal(u8, out)


def test_int64_values_outside_the_byte_range_are_converted_as_float_does():
    ids = torch.tensor([[-5, 300, 70000, 12, 0, 255, -100000, 9], [1, 2, 3, 4, 5, 6, 7, 1 << 30]], dtype=torch.int64)
    bands = torch.tensor([1.0, 0.5, 2.0, 1.5])
    out = pkg().byte_features(ids, bands, 8)
    e, _ = bc.compare(out.numpy(), ids.numpy(), bands.numpy(), 8)
    assert e <= bc.TOL_FACTOR * bc.r_ref()


@pytest.mark.parametrize("name", bc.EMBEDDING_FIXTURES[:3] + bc.ENCODER_FIXTURES)
def test_modules_load_the_reference_state_dict_and_reproduce_its_output(name):
    z = load_golden(name)
    p = pkg()
    if name in bc.ENCODER_FIXTURES:
        M = int(z["width"]) // 2
        mod = p.ByteSpectralEncoder(z["sd.freq_to_embed.3.weight"].shape[0], max_freq_components=M)
    else:
        mod = p.ByteSpectralEmbedding(int(z["width"]), max_seq_len=z["ids"].shape[1])
    mod.load_state_dict(sd_of(z), strict=True)
    ids = torch.from_numpy(z["ids"])
    y = mod.eval()(ids)
    assert y.shape == (ids.shape[0], ids.shape[1], mod.embed_dim)
    if name in bc.ENCODER_FIXTURES:
        assert y.stride(1) == 0                                     # an expanded view, as in the reference
        y = y[:, :1]
    e = rel_err(y.detach().numpy(), z["y"])
    print(f"{name}: output vs reference {e:.3e}")
    assert e <= TOL_ACT


def test_language_model_has_the_reference_layout():
    z = load_golden(bc.LM_FIXTURE)
    m = pkg().SpectralLanguageModel(embed_dim=32, num_layers=2, max_seq_len=64, dropout=0.1)
    m.load_state_dict(sd_of(z), strict=True)
    keys = set(m.state_dict())
    assert {"byte_encoder.freq_bands", "byte_encoder.freq_proj.0.weight", "byte_encoder.freq_proj.1.bias",
            "byte_encoder.freq_proj.3.weight", "layers.1.spectral_mix.weight_real", "norm.weight", "output.bias"} <= keys
    d = pkg().SpectralLanguageModel()
    assert (d.embed_dim, len(d.layers), d.max_seq_len, d.dropout.p) == (256, 6, 512, 0.1)
    assert d.byte_encoder.freq_bands.shape == (128,) and d.output.out_features == 256
    e = pkg().ByteSpectralEncoder()
    assert e.freq_weights.shape == (512,) and e.freq_to_embed[0].in_features == 1024


def test_band_gradient_against_autograd_through_the_position_loop():
    g = torch.Generator().manual_seed(5)
    for (B, T, W) in [(2, 10, 12), (2, 16, 8), (3, 9, 32)]:
        ids = torch.randint(0, 256, (B, T), generator=g, dtype=torch.int64)
        up = torch.randn(B, T, W, generator=g)
        bands = (torch.rand(W // 2, generator=g) + 0.5).requires_grad_(True)
        out = pkg().byte_features(ids, bands, W)
        out.backward(up)
        b64 = bands.detach().double().requires_grad_(True)
        ref = bc.loop64(ids.numpy(), b64, W)
        assert rel_err(out.detach().numpy(), ref.detach().numpy()) <= TOL_ACT
        ref.backward(up.double())
        assert bands.grad.shape == bands.shape
        assert rel_err(bands.grad.numpy(), b64.grad.numpy()) <= TOL_PARAM
        assert not bands.grad[min(W // 2, T // 2):].any()


def test_constant_row_is_finite_with_unit_phasors():
    ids = torch.full((2, 16), 65, dtype=torch.int64)
    ids[1] = 255
    out = pkg().byte_features(ids, torch.ones(12), 24)             # k = 8: all three blocks
    assert torch.isfinite(out).all()
    s, c = out[..., 8:16], out[..., 16:24]
    assert torch.allclose(s * s + c * c, torch.ones_like(s), atol=1e-6)
    assert torch.allclose(out[..., 0], (ids[:, :1].float() / 127.5 - 1).abs() * 16, rtol=1e-6)


def test_single_byte_rows_are_all_zero():
    out = pkg().byte_features(torch.tensor([[7], [200]]), torch.ones(4), 8)
    assert out.shape == (2, 1, 8) and not out.any()
    enc = pkg().byte_features(torch.tensor([[7], [200]]), torch.ones(4), 8, positions=False)
    assert enc.shape == (2, 8) and not enc.any()
    assert pkg().byte_features(torch.zeros((0, 5), dtype=torch.uint8), torch.ones(4), 8).shape == (0, 5, 8)


def test_argument_checks():
    bf = pkg().byte_features
    with pytest.raises(TypeError):
        bf(torch.zeros(2, 3), torch.ones(4), 8)
    with pytest.raises(TypeError):
        bf(torch.zeros(6, dtype=torch.uint8), torch.ones(4), 8)
    with pytest.raises(ValueError):
        bf(torch.zeros(2, 16, dtype=torch.uint8), torch.ones(2), 8)          # 4 bins, 2 weights
    with pytest.raises(ValueError):
        bf(torch.zeros(2, 16, dtype=torch.uint8), torch.ones(4), 0)
    with pytest.raises(ValueError):
        bf(torch.zeros(2, 16, dtype=torch.uint8), torch.ones(4), 8, native=True)   # no native launch on the CPU


def test_stop_rule_keeps_up_to_the_first_stop_byte():
    cut = pkg().SpectralLanguageModel.cut_at_stop
    assert cut(3, [200, 0, 65, 66, 67, 0, 68]) == [200, 0, 65, 66, 67, 0]         # the prompt's own bytes never stop it
    assert cut(2, [65, 66, 67, 68, 130, 69, 0]) == [65, 66, 67, 68, 130]
    assert cut(2, [65, 66, 67, 68]) == [65, 66, 67, 68]
    assert cut(2, [65, 66, 127, 128]) == [65, 66, 127, 128]
    assert cut(1, [65, 0]) == [65, 0]
    dec = pkg().SpectralLanguageModel.decode
    assert dec([72, 105, 233]) == "Hi\xe9" and dec([72, 0]) == "H\x00"


def test_generation_is_deterministic_under_a_seeded_generator():
    torch.manual_seed(3)
    m = pkg().SpectralLanguageModel(embed_dim=16, num_layers=0, max_seq_len=8)    # (the mixing layers have no CPU path)
    with torch.no_grad():
        m.output.weight.mul_(4.0)
        m.output.bias[:32] = -30.0                                                # keep the draws in the text range
        m.output.bias[127:] = -30.0
    run = lambda seed, **kw: m.generate("spectral", max_new_bytes=12, generator=torch.Generator().manual_seed(seed), **kw)
    a = run(11)
    assert a == run(11) and a.startswith("spectral") and len(a) == 8 + 12
    assert any(run(s) != a for s in (12, 13, 14))
    ids = m.generate_ids([ord(c) for c in "ab"], 5, 0.7, torch.Generator().manual_seed(1))
    assert ids[:2] == [97, 98] and len(ids) == 7 and all(32 <= v < 127 for v in ids[2:])
    with pytest.raises(ValueError):
        m.generate("", 3)
