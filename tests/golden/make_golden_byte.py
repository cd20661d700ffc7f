#!/usr/bin/env python3
"""Golden vectors of the byte-spectral models, produced by the REFERENCE modules on CPU
(fft_tensor/byte_spectral_model.py:20-161 ByteSpectralEmbedding / SpectralLanguageModel,
fft_tensor/byte_spectral.py:20-108 ByteSpectralEncoder).  Every parameter randomised; freq_bands and freq_weights come
from U(0.5, 1.5), so that a missing multiply shows.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_byte.py

Every fixture records ids, bands (the band weights), width, `features` (what the reference hands to its projection,
caught by a hook), and -- but for the features-only case -- the state_dict and the module's output.  The ids of a case
are redrawn (seed + 1, + 2, ...) until every kept bin has |S| >= 2 MIN_MAG in float64: no fixture leaves out a bin by the
rule of tests/byte_common.py.  The generator prints the reference's own normalised error against the float64 table.
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
import byte_common as bc                                     # noqa: E402

from fft_tensor.byte_spectral_model import ByteSpectralEmbedding, SpectralLanguageModel   # noqa: E402
from fft_tensor.byte_spectral import ByteSpectralEncoder     # noqa: E402


def conditioned_ids(B, T, k):
    seed = SEED
    while True:
        ids = torch.randint(0, 256, (B, T), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
        if k == 0 or float(np.abs(bc.spectrum64(ids.numpy(), k)).min()) >= 2 * bc.MIN_MAG:
            return ids
        seed += 1


def run(name, mod, proj, bands, ids, width, positions, keep_sd=True):
    mg._randomize(mod)
    with torch.no_grad():
        bands.uniform_(0.5, 1.5)
    caught = []
    h = proj.register_forward_pre_hook(lambda m, a: caught.append(a[0].detach().clone()))
    mod.eval()
    with torch.no_grad():
        y = mod(ids)
    h.remove()
    rec = {"ids": ids, "bands": bands.detach(), "width": np.int64(width), "features": caught[0]}
    if keep_sd:
        rec["y"] = y[:, :1] if not positions else y          # the encoder's output is one row expanded over T
        for k, v in mod.state_dict().items():
            rec["sd." + k] = v
    e, share = bc.compare(caught[0].numpy(), ids.numpy(), bands.detach().numpy(), width, positions)
    assert share == 0.0
    print(f"{name}: reference vs float64 table {e:.3e}")
    mg.save(name, rec)
    assert os.path.getsize(os.path.join(mg.OUT, name + ".npz")) < 512 * 1024


def embedding_case(name, B, T, D, keep_sd=True):
    torch.manual_seed(SEED)
    mod = ByteSpectralEmbedding(D, max_seq_len=T)
    run(name, mod, mod.freq_proj, mod.freq_bands, conditioned_ids(B, T, min(D // 2, T // 2)), D, True, keep_sd)


def encoder_case(name, B, T, M, D=24):
    torch.manual_seed(SEED)
    mod = ByteSpectralEncoder(D, max_freq_components=M)
    run(name, mod, mod.freq_to_embed, mod.freq_weights, conditioned_ids(B, T, min(M, T // 2)), 2 * M, False)


def lm_case(name, B, T, D, layers):
    torch.manual_seed(SEED)
    mod = SpectralLanguageModel(embed_dim=D, num_layers=layers, max_seq_len=T, dropout=0.1)
    enc = mod.byte_encoder
    run(name, mod, enc.freq_proj, enc.freq_bands, conditioned_ids(B, T, min(D // 2, T // 2)), D, True)


if __name__ == "__main__":
    embedding_case(bc.EMBEDDING_FIXTURES[0], 2, 64, 32)                  # T >= D: the cosine block is dropped
    embedding_case(bc.EMBEDDING_FIXTURES[1], 2, 37, 32)                  # odd T
    embedding_case(bc.EMBEDDING_FIXTURES[2], 3, 10, 12)                  # 2k < D < 3k: the cosine block cut part-way
    embedding_case(bc.EMBEDDING_FIXTURES[3], 1, 512, 64, keep_sd=False)  # the default length, features only
    encoder_case(bc.ENCODER_FIXTURES[0], 2, 100, 16)                     # k = M: cut at 2 M
    encoder_case(bc.ENCODER_FIXTURES[1], 2, 20, 16)                      # k = 10 < M: the row is padded
    lm_case(bc.LM_FIXTURE, 2, 64, 32, 2)
