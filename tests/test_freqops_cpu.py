"""The mirror of fft_tensor.frequency_ops without a GPU: names, the declared entries, and the CPU path -- the reference's
own torch ops -- against the goldens the reference produced (tests/golden/make_golden_freqops.py).

Both sides run the same torch ops on the same machine kind, so the bound is 1e-6 max-normalised.  Measured distances (CPU,
torch 2.x): 0 for every golden of the attention, the layernorm, the layer, the embedding methods and circulant_matmul
(the op sequences are identical) and for frequency_relu against the recorded result; frequency_relu against its own
input (it is the identity up to rounding): 1.2e-7."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

import freqops_common as fc
import tensor_cuda_fft_amd as pkg
from tensor_cuda_fft_amd import _lib, frequency_ops as fo, functional as fn

SAME_OPS = 1e-6


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _close(got, want, what=""):
    if isinstance(want, torch.Tensor):
        want = want.detach().resolve_conj().numpy()
    e = rel_err(got.detach().resolve_conj().numpy(), np.asarray(want))
    print(f"{what} rel_err {e:.3g}")
    assert e <= SAME_OPS, (what, e)


def test_names_are_exported():
    for name in ("FrequencyAttention", "FrequencyMatMul", "FrequencyTransformerLayer", "ComplexSemanticEmbedding",
                 "frequency_relu", "frequency_layernorm", "frequency_attention"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    assert pkg.FrequencyTransformerLayer is fo.FrequencyTransformerLayer
    for member in ("frequency_attention", "fnet_attention"):
        assert hasattr(pkg.FrequencyAttention, member)
    for member in ("circulant_matmul", "block_streaming_matmul"):
        assert hasattr(pkg.FrequencyMatMul, member)
    assert "out of scope" not in fo.__doc__


def test_entries_are_declared_and_bound():
    """The three entries are part of the C ABI -- declared in include/smx_freq.h, which smx.h includes -- and bound by
    _lib from that header (_SIGS_EXT: smx.h's own table, _SIGS, is recorded as it stood and does not grow).  Their derived
    signatures equal the recorded tests/golden/abi_signatures_ext.txt line for line."""
    import ctypes
    import os
    from conftest import GOLDEN
    inc = os.path.dirname(_lib.HEADER_PATH)
    assert '#include "smx_freq.h"' in open(_lib.HEADER_PATH).read()
    text = open(os.path.join(inc, "smx_freq.h")).read()
    entries = ("smx_freq_attention_forward", "smx_freq_attention_workspace_bytes", "smx_freq_layernorm_forward")
    for entry in entries:
        assert f"int {entry}(" in text
        assert entry in _lib._SIGS_EXT and entry not in _lib._SIGS and entry not in _lib._SINCE
    assert tuple(sorted(_lib._SIGS_EXT)) == entries
    assert _lib.SMX_VERSION == 303
    assert _lib.SMX_FREQ_LN_MAX_D == fn.FREQ_LN_MAX_D == 1024
    codes = {ctypes.c_int: "i", ctypes.c_longlong: "q", ctypes.c_float: "f", ctypes.c_void_p: "P", ctypes.c_size_t: "z"}

    def spell(t):
        return codes[t] if t in codes else "[" + codes[t._type_] + "]"
    got = [f"{n} {spell(r)}({''.join(spell(a) for a in args)})" for n, (r, args) in sorted(_lib._SIGS_EXT.items())]
    got += [f"const {n} {v}" for n, v in sorted(_lib._DEFINES_EXT.items())]
    assert got == open(os.path.join(GOLDEN, "abi_signatures_ext.txt")).read().splitlines()


def test_a_missing_extension_header_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "smx.h"))
    with pytest.raises(_lib.SmxError, match="smx_freq.h not found"):
        _lib._read_ext_headers()


@pytest.mark.parametrize("name", ["U01_fattn_2x2x8x4", "U02_fattn_1x3x65x3_t05"])
def test_attention_cpu_path_equals_the_golden(name):
    g = load_golden(name)
    q, k, v, temp = _t(g["q"]), _t(g["k"]), _t(g["v"]), float(g["temperature"])
    _close(pkg.FrequencyAttention.frequency_attention(q, k, v, temp), g["out"], name)
    _close(fn.frequency_attention(q, k, v, temp, merge_heads=True), fc.merge_heads(_t(g["out"])), name + " merged")
    assert float(g["ref_err_out"]) <= 2.5e-6


@pytest.mark.parametrize("name", ["U03_fln_2x8x4", "U04_fln_2x7x3_zeros", "U05_fln_2x9x130"])
def test_layernorm_and_relu_cpu_path_equal_the_golden(name):
    g = load_golden(name)
    z = _t(g["z"])
    _close(pkg.frequency_layernorm(z, float(g["eps"])), g["out"], name)
    _close(pkg.frequency_relu(z), g["relu"], name + " relu")
    _close(pkg.frequency_relu(z), g["z"], name + " relu is the identity")


@pytest.mark.parametrize("name", ["U06_flayer_2x33x64_h4", "U07_flayer_1x5x6_h3"])
def test_layer_cpu_path_equals_the_golden(name):
    g = load_golden(name)
    x = _t(g["x"])
    layer = pkg.FrequencyTransformerLayer(x.shape[-1], int(g["heads"]), device="cpu")
    for attr in ("q_proj_freq", "k_proj_freq", "v_proj_freq", "o_proj_freq"):
        w = getattr(layer, attr)
        assert w.dtype == torch.complex64 and w.shape == (x.shape[-1],) * 2 and not isinstance(w, torch.nn.Parameter)
        assert 0.015 < float(torch.view_as_real(w).std()) * 2 ** 0.5 < 0.025 or w.numel() < 100      # randn * 0.02
        setattr(layer, attr, _t(g["w" + attr[0]]))
    out = layer.forward(x)
    assert out.shape == x.shape and out.is_contiguous()
    _close(out, g["out"], name)
    layer.o_proj_freq = layer.o_proj_freq * 2                # reassigned between calls: nothing derived is kept
    _close(layer.forward(x), 2 * g["out"], name + " reassigned")


def test_embedding_mirrors_the_reference():
    g = load_golden("U08_embedding_50x16")
    torch.manual_seed(1234)                                  # the generator's SEED: the CPU generator draws the same table
    emb = pkg.ComplexSemanticEmbedding(50, 16, device="cpu")
    assert (emb.vocab_size, emb.embed_dim, emb.device) == (50, 16, "cpu")
    _close(emb.freq_embeddings, g["freq_embeddings"], "table from the same seed")
    emb.freq_embeddings = _t(g["freq_embeddings"])
    ids = _t(g["ids"])
    e = emb.lookup(ids)
    _close(e, g["lookup"], "lookup")
    _close(emb.semantic_similarity(e[0], e[1]), g["similarity"], "similarity")
    _close(emb.phase_relationship(e[0], e[1]), g["phase"], "phase")


def test_circulant_matmul_layouts_and_errors():
    g = load_golden("U09_circulant_2x5x12x20")
    x = _t(g["x"])
    cm = pkg.FrequencyMatMul.circulant_matmul
    y = cm(x, _t(g["w_out_in"]))
    assert y.shape == (2, 5, 20)
    _close(y, g["out_out_in"], "(D_out, D_in)")
    y = cm(x, _t(g["w_k_n"]))
    assert y.shape == (2, 5, 20)
    _close(y, g["out_k_n"], "(K, N)")
    with pytest.raises(ValueError) as e:
        cm(x, torch.zeros(7, 9, dtype=torch.complex64))
    assert str(e.value) == "Dimension mismatch: x has 12, w_freq is torch.Size([7, 9])"
    with pytest.raises(ValueError) as e:
        cm(x, torch.zeros(12, dtype=torch.complex64))
    assert str(e.value) == "Unexpected w_freq shape: torch.Size([12])"


def test_gradients_through_the_cpu_path_equal_the_compositions():
    gen = torch.Generator().manual_seed(5)
    q, k, v = (fc.crandn(gen, 2, 2, 6, 3).requires_grad_(True) for _ in range(3))
    go = fc.crandn(gen, 2, 2, 6, 3)
    got = torch.autograd.grad(pkg.FrequencyAttention.frequency_attention(q, k, v, 0.7), (q, k, v), go)
    want = torch.autograd.grad(fc.attention_ref(q, k, v, 0.7), (q, k, v), go)
    for a, b, n in zip(got, want, "qkv"):
        _close(a, b, "grad_" + n)
    z = fc.crandn(gen, 3, 5, 6).requires_grad_(True)
    gz = fc.crandn(gen, 3, 5, 6)
    got, = torch.autograd.grad(pkg.frequency_layernorm(z, 1e-3), z, gz)
    want, = torch.autograd.grad(fc.layernorm_ref(z, 1e-3), z, gz)
    _close(got, want, "grad_z")


def test_edge_values():
    out = pkg.frequency_layernorm(torch.ones(3, 1, dtype=torch.complex64))
    assert out.shape == (3, 1) and bool(torch.isnan(torch.view_as_real(out)).all())         # D = 1: NaN, as the reference
    zero = torch.zeros(4, dtype=torch.complex64)
    assert bool((pkg.frequency_relu(zero) == 0).all())
    z = torch.tensor([[0j, 3 + 4j, 1j]], dtype=torch.complex64)                              # the phase of 0 is 0
    out = pkg.frequency_layernorm(z)
    m = torch.tensor([0.0, 5.0, 1.0])
    want = (m - m.mean()) / (m.std() + 1e-5)
    assert abs(float(out[0, 0].real) - float(want[0])) < 1e-6 and float(out[0, 0].imag) == 0.0
