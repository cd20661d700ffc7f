#!/usr/bin/env python3
"""Golden vectors of fft_tensor/frequency_ops.py, produced by the REFERENCE module on the CPU: frequency_attention,
frequency_layernorm, frequency_relu, FrequencyTransformerLayer (weights recorded), ComplexSemanticEmbedding (its table
recorded, so that a test can inject it) and circulant_matmul in both weight layouts.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_freqops.py [name prefixes]

Beside the reference's fp32 result every fixture records `ref_err_out`: its max-normalised error against the complex128
evaluation of tests/freqops_common.py.  The generator FAILS if that exceeds a quarter of TOL_ACT, or if the restatement
in fp32 is further than 2e-6 from the reference: the yardstick is never outside its own bound.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                     # noqa: E402  (puts the reference on sys.path)
from make_golden import SEED                                 # noqa: E402
import freqops_common as fc                                  # noqa: E402
from conftest import TOL_ACT, rel_err                        # noqa: E402

from fft_tensor import frequency_ops as ref                  # noqa: E402


def _checked(name, out, again, out64):
    """the record entries of one output: the restatement reproduces it, and its own error is inside the bound"""
    assert rel_err(again.numpy(), out.numpy()) <= 2e-6, name
    e = rel_err(out.numpy(), out64.numpy())
    assert e <= TOL_ACT / 4, (name, e)
    return {"out": out, "ref_err_out": np.float64(e)}


def attention_case(name, B, H, N, D, temperature=1.0):
    gen = torch.Generator().manual_seed(SEED)
    q, k, v = (fc.crandn(gen, B, H, N, D) for _ in range(3))
    out = ref.FrequencyAttention.frequency_attention(q, k, v, temperature)
    rec = _checked(name, out, fc.attention_ref(q, k, v, temperature),
                   fc.attention_ref(fc.wide(q), fc.wide(k), fc.wide(v), temperature))
    rec.update({"q": q, "k": k, "v": v, "temperature": np.float64(temperature)})
    mg.save(name, rec)


def layernorm_case(name, shape, eps=1e-5, zeros=False):
    gen = torch.Generator().manual_seed(SEED)
    z = fc.crandn(gen, *shape)
    if zeros:
        z[..., 0, 1] = 0                                     # exact zeros: their phase is 0
    out = ref.frequency_layernorm(z, eps)
    rec = _checked(name, out, fc.layernorm_ref(z, eps), fc.layernorm_ref(fc.wide(z), eps))
    rec.update({"z": z, "eps": np.float64(eps), "relu": ref.frequency_relu(z)})
    mg.save(name, rec)


def layer_case(name, B, N, d_model, heads):
    torch.manual_seed(SEED)
    layer = ref.FrequencyTransformerLayer(d_model, heads, device="cpu")
    gen = torch.Generator().manual_seed(SEED + 1)
    x = fc.crandn(gen, B, N, d_model)
    w = [layer.q_proj_freq, layer.k_proj_freq, layer.v_proj_freq, layer.o_proj_freq]
    out = layer.forward(x)
    rec = _checked(name, out, fc.layer_ref(x, *w, heads), fc.layer_ref(fc.wide(x), *(fc.wide(t) for t in w), heads))
    rec.update({"x": x, "wq": w[0], "wk": w[1], "wv": w[2], "wo": w[3], "heads": np.int64(heads)})
    mg.save(name, rec)


def embedding_case(name, vocab, dim, B, N):
    torch.manual_seed(SEED)
    emb = ref.ComplexSemanticEmbedding(vocab, dim, device="cpu")
    gen = torch.Generator().manual_seed(SEED + 1)
    ids = torch.randint(0, vocab, (B, N), generator=gen)
    e = emb.lookup(ids)
    mg.save(name, {"freq_embeddings": emb.freq_embeddings, "ids": ids, "lookup": e,
                   "similarity": emb.semantic_similarity(e[0], e[1]), "phase": emb.phase_relationship(e[0], e[1])})


def circulant_case(name, B, M, K, N):
    gen = torch.Generator().manual_seed(SEED)
    x = torch.randn(B, M, K, generator=gen)
    w_out_in, w_k_n = fc.crandn(gen, N, K), fc.crandn(gen, K, N)
    rec = {"x": x, "w_out_in": w_out_in, "w_k_n": w_k_n,
           "out_out_in": ref.FrequencyMatMul.circulant_matmul(x, w_out_in),
           "out_k_n": ref.FrequencyMatMul.circulant_matmul(x, w_k_n)}
    for key, w in (("out_out_in", w_out_in), ("out_k_n", w_k_n)):
        assert rel_err(fc.circulant_ref(x, w).numpy(), rec[key].numpy()) <= 2e-6, key
    mg.save(name, rec)


if __name__ == "__main__":
    only = sys.argv[1:]
    if only:
        _save = mg.save
        mg.save = lambda name, rec: _save(name, rec) if any(name.startswith(p) for p in only) else None
    attention_case("U01_fattn_2x2x8x4", 2, 2, 8, 4)
    attention_case("U02_fattn_1x3x65x3_t05", 1, 3, 65, 3, temperature=0.5)
    layernorm_case("U03_fln_2x8x4", (2, 8, 4))
    layernorm_case("U04_fln_2x7x3_zeros", (2, 7, 3), eps=1e-3, zeros=True)
    layernorm_case("U05_fln_2x9x130", (2, 9, 130))
    layer_case("U06_flayer_2x33x64_h4", 2, 33, 64, 4)
    layer_case("U07_flayer_1x5x6_h3", 1, 5, 6, 3)
    embedding_case("U08_embedding_50x16", 50, 16, 2, 7)
    circulant_case("U09_circulant_2x5x12x20", 2, 5, 12, 20)
