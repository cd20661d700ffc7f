#!/usr/bin/env python3
"""Golden vectors of the enhanced spectral block and its members, produced by the REFERENCE modules on CPU
(fft_tensor/spectral_enhancements.py: RotaryFrequencyEmbedding :20-71, GatedSpectralUnit :74-116,
CausalFrequencyMask :169-211, EnhancedSpectralBlock :278-333).  Dropout 0, every parameter randomised
(LayerNorm affines and phase filters included).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_enhanced.py [name prefixes]

Names start with E: the layer tests glob G*.npz and H*.npz.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                     # noqa: E402  (puts the reference on sys.path)
from make_golden import SEED, _module_case, _randomize      # noqa: E402


def enhanced_case(name, B, T, D):
    from fft_tensor.spectral_enhancements import EnhancedSpectralBlock
    torch.manual_seed(SEED)
    blk = EnhancedSpectralBlock(D, dropout=0.0)
    _randomize(blk)
    _module_case(name, blk, torch.randn(B, T, D), torch.randn(B, T, D))


def rope_case(name, B, T, D):
    from fft_tensor.spectral_enhancements import RotaryFrequencyEmbedding
    torch.manual_seed(SEED)
    _module_case(name, RotaryFrequencyEmbedding(D), torch.randn(B, T, D), torch.randn(B, T, D))


def gsu_case(name, B, T, D):
    from fft_tensor.spectral_enhancements import GatedSpectralUnit
    torch.manual_seed(SEED)
    m = GatedSpectralUnit(D)
    _randomize(m)
    _module_case(name, m, torch.randn(B, T, D), torch.randn(B, T, D))


def causal_case(name, B, T, D):
    from fft_tensor.spectral_enhancements import CausalFrequencyMask
    torch.manual_seed(SEED)
    _module_case(name, CausalFrequencyMask(), torch.randn(B, T, D), torch.randn(B, T, D))


if __name__ == "__main__":
    only = sys.argv[1:]
    if only:
        _save = mg.save
        mg.save = lambda name, rec: _save(name, rec) if any(name.startswith(p) for p in only) else None
    enhanced_case("E01_enh_2x256x32", 2, 256, 32)
    enhanced_case("E02_enh_2x100x16", 2, 100, 16)            # T % 8 != 0
    enhanced_case("E03_enh_1x1024x8", 1, 1024, 8)            # 513 bins
    enhanced_case("E04_enh_3x40x6", 3, 40, 6)                # D % 4 == 2
    rope_case("E11_rope_2x300x34", 2, 300, 34)
    gsu_case("E21_gsu_2x64x24", 2, 64, 24)
    causal_case("E31_causal_2x50x8", 2, 50, 8)
