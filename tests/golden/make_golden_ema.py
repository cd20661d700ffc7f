#!/usr/bin/env python3
"""Golden vectors of the SpectralEMA scan and of ChunkLM(use_ema=True), produced by the REFERENCE modules on CPU
(fft_lm/spectral_ssm.py:38-125 SpectralEMA, fft_lm/chunk_head.py:16-69 ChunkLM).  Every parameter randomised
(rho_logit ~ N(2, 1), theta_raw ~ N(0, 0.5)).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ema.py [name prefixes]

Beside the reference's fp32 results every fixture records `ref_err_<output>`: the max-normalised error of that fp32
result against an fp64 evaluation of the same op sequence (tests/ema_common.py -- the reference's step pins fp32, so
its fp64 run is a restatement, checked here to reproduce the reference in fp32).  The generator FAILS if one of them
exceeds a quarter of the tolerance the tests apply to that output: the yardstick is never outside its own bound.
Byte inputs: every chunk with a bin |X| < 0.25 is redrawn (the reference follows the phase of rounding noise there).
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
import ema_common as ec                                      # noqa: E402
from conftest import TOL_ACT, TOL_PARAM, rel_err             # noqa: E402

from fft_lm.spectral_ssm import EMAConfig, SpectralEMA       # noqa: E402
from fft_lm.chunk_head import ChunkLM                        # noqa: E402


def _tol(key):
    return TOL_ACT if key in ("state", "grad_chunks", "grad_init", "y") else TOL_PARAM


def _record_errors(rec, ref64):
    for k, v64 in ref64.items():
        e = rel_err(rec[k].detach().numpy(), v64.detach().numpy())
        assert e <= _tol(k if not k.startswith("grad.") else "param") / 4, (k, e)
        rec["ref_err_" + k] = np.float64(e)


def scan_case(name, mode, B, S, F, with_init=False, zeros=True):
    torch.manual_seed(SEED)
    ema = SpectralEMA(EMAConfig(n_freqs=F, mode=mode))
    with torch.no_grad():
        ema.rho_logit.copy_(2.0 + torch.randn(F))
        ema.theta_raw.copy_(0.5 * torch.randn(F))
    chunks = torch.randn(B, S, F, dtype=torch.complex64)
    if zeros and S > 2:
        chunks[B - 1, S // 2] = 0                            # one chunk exactly 0+0j
        chunks[0, 0, F // 2] = 0                             # one zero bin on the zero state: the state stays exactly zero
    init = torch.randn(B, F, dtype=torch.complex64) if with_init else None
    g = torch.randn(B, F, dtype=torch.complex64)

    def run(fn, cdt, rl, tr):
        c = chunks.clone().to(cdt).requires_grad_(True)
        i0 = None if init is None else init.clone().to(cdt).requires_grad_(True)
        y = fn(c, i0, rl, tr)
        y.backward(g.to(cdt))
        out = {"state": y.detach(), "grad_chunks": c.grad, "grad_rho_logit": rl.grad}
        if i0 is not None:
            out["grad_init"] = i0.grad
        if mode == "aligned":
            out["grad_theta_raw"] = tr.grad
        else:
            assert tr.grad is None                           # polar: theta_raw takes no part
        return out

    rec = run(lambda c, i0, rl, tr: ema.scan(c, i0), torch.complex64, ema.rho_logit, ema.theta_raw)
    rl64 = ema.rho_logit.detach().double().requires_grad_(True)
    tr64 = ema.theta_raw.detach().double().requires_grad_(True)
    ref64 = run(lambda c, i0, rl, tr: ec.scan_ref(c, rl, tr, mode, i0), torch.complex128, rl64, tr64)
    # the restatement is the reference's sequence: in fp32 it lands on the reference's own numbers
    rl32 = ema.rho_logit.detach().clone().requires_grad_(True)
    tr32 = ema.theta_raw.detach().clone().requires_grad_(True)
    again = run(lambda c, i0, rl, tr: ec.scan_ref(c, rl, tr, mode, i0), torch.complex64, rl32, tr32)
    for k in rec:
        assert rel_err(again[k].numpy(), rec[k].numpy()) <= 2e-6, (name, k)
    _record_errors(rec, ref64)
    rec.update({"chunks": chunks, "g": g, "mode": np.array(mode), "sd.rho_logit": ema.rho_logit.detach(),
                "sd.theta_raw": ema.theta_raw.detach()})
    if init is not None:
        rec["init"] = init
    mg.save(name, rec)


def chunklm_case(name, B, T, L, chunk, mode="aligned"):
    torch.manual_seed(SEED)
    gen = torch.Generator().manual_seed(SEED)
    model = ChunkLM(ec.StubBackbone(8), chunk, use_ema=True, ema_chunk_len=L, ema_mode=mode)
    F = L // 2 + 1
    with torch.no_grad():
        model.ema.rho_logit.copy_(2.0 + torch.randn(F))
        model.ema.theta_raw.copy_(0.5 * torch.randn(F))
        model.ema_proj.weight.normal_(0.0, 0.3)
        model.ema_proj.bias.normal_(0.0, 0.1)
        model.head.weight.normal_(0.0, 0.1)
        model.head.bias.normal_(0.0, 0.1)
    x = ec.conditioned_bytes(gen, B, T, L)
    assert float(ec.byte_chunks(x, L).abs().min()) >= ec.MIN_BIN
    g = torch.randn(B, chunk, 256)
    y = model(x)
    y.backward(g)
    rec = {"y": y.detach()}
    for k, p in model.named_parameters():
        rec["grad." + k] = p.grad
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in model.state_dict().items()}
    y64 = ec.chunklm_ref(sd64, x, L, chunk, mode)
    y64.backward(g.double())
    ref64 = {"y": y64.detach()}
    ref64.update({"grad." + k: sd64[k].grad for k, _ in model.named_parameters()})
    _record_errors(rec, ref64)
    rec.update({"x": x, "g": g, "L": np.int64(L), "chunk": np.int64(chunk), "mode": np.array(mode)})
    for k, v in model.state_dict().items():
        rec["sd." + k] = v
    mg.save(name, rec)


if __name__ == "__main__":
    only = sys.argv[1:]
    if only:
        _save = mg.save
        mg.save = lambda name, rec: _save(name, rec) if any(name.startswith(p) for p in only) else None
    scan_case("S01_ema_aligned_3x64x9", "aligned", 3, 64, 9)             # the chunk head's own shape
    scan_case("S02_ema_polar_2x37x33", "polar", 2, 37, 33)
    scan_case("S03_ema_init_2x5x130", "aligned", 2, 5, 130, with_init=True, zeros=False)   # B F % 64 != 0
    scan_case("S04_ema_update_2x1x9", "aligned", 2, 1, 9, with_init=True, zeros=False)     # one step from a state
    chunklm_case("C01_chunklm_2x64", 2, 64, 16, 4)
    chunklm_case("C02_chunklm_2x100_L12", 2, 100, 12, 4)                 # 8 chunks, 4 trailing bytes
