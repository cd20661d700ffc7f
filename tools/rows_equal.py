#!/usr/bin/env python3
"""Do two builds of libsmx.so compute the SAME BITS in the row kernels (csrc/smx_rows.h and its three users)?

    python tools/rows_equal.py --libs libsmx_parent.so,libsmx.so [--family block|enhanced|sln|gate|mix]

Both builds are loaded into one process (as tools/ab_inproc.py does) and fed the same seeded inputs, in eval and with
dropout, at one width per instantiated (VEC, CH) class of each family -- the odd and D % 4 != 0 classes included:
  block     smx_block_forward / _backward: y, spectrum, LayerNorm statistics, grad_x, parameter gradients, gamma / beta
  enhanced  the three lines rope_norm, residual_norm, gate_blend (and rope_rotate), forward and backward
  sln       spectral_layer_norm forward and backward, interleaved and planar
  gate, mix spectral_gate and mix_paths, forward and backward
Every comparison is of the bit patterns (torch.equal on the int32 view: signed zeros count).  One JSON line per case;
exit status 1 if any case differs or fails."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensor_cuda_fft_amd as pkg                                   # noqa: E402,F401
from tensor_cuda_fft_amd import _lib, functional as fn              # noqa: E402

DEV = torch.device("cuda:0")


def bits(t):
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32)


def rnd(*shape, cplx=False):
    return torch.randn(*shape, device=DEV, dtype=torch.complex64 if cplx else torch.float32)


def grads(outs, leaves):
    """outputs and the gradients of sum(out * fixed cotangent) in every leaf"""
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    gen = torch.Generator(device=DEV).manual_seed(7)
    cots = [torch.randn(o.shape, device=DEV, dtype=o.dtype, generator=gen) if not o.is_complex() else
            torch.view_as_complex(torch.randn(o.shape + (2,), device=DEV, generator=gen)) for o in outs]
    g = torch.autograd.grad(outs, leaves, cots, allow_unused=True)
    return list(outs) + [x for x in g if x is not None]


def case_block(D, p):
    B, N, F = 2, 256, min(D // 2, 64)
    x, g = rnd(B, N, D) + 0.5, rnd(B, N, D)
    lw, lb = 1 + 0.3 * rnd(D), 0.2 * rnd(D)
    wr, wi, bias = 1 + 0.5 * rnd(D, F), 0.5 * rnd(D, F), 0.1 * rnd(D)
    rng = torch.tensor([1234567, 89], dtype=torch.int64, device=DEV) if p else None
    y, xk, st = fn.block_forward_raw(x, lw, lb, 1e-5, wr, wi, bias, dropout_p=p, rng=rng)
    gx, flat, lnf = fn.block_backward_raw(g, x, st, lw, xk, wr, wi, dropout_p=p, rng=rng)
    return [y, xk, st, gx, flat, lnf]


def case_enhanced(D, p):
    B, T = 3, 37
    leaves = [t.requires_grad_(True) for t in (rnd(B, T, D) + 0.5, rnd(B, T, D), rnd(B, T, 2 * D), rnd(B, T, D))]
    x, pin, a, v = leaves
    par = [t.requires_grad_(True) for t in (1 + 0.3 * rnd(D), 0.2 * rnd(D), 1 + 0.3 * rnd(D), 0.2 * rnd(D),
                                            1 + 0.3 * rnd(D), 0.2 * rnd(D), 1 + 0.3 * rnd(2 * D), 0.2 * rnd(2 * D))]
    w1, b1, w2, b2, w3, b3, wg, bg = par
    ang = rnd(64, D // 2)
    rot = torch.polar(torch.ones_like(ang), ang)
    ds = fn.DropoutState(DEV) if p else None
    outs = list(fn.rope_norm(x, rot, w1, b1, w2, b2, 1e-5, 1e-6, p, ds))
    outs += list(fn.residual_norm(x, pin, w3, b3, 1e-5, p, ds))
    outs += [fn.gate_blend(a, v, x, wg, bg, 1e-5, p, ds), fn.gate_blend(a, v, None, wg, bg, 1e-5, p, ds)]
    if not p:
        outs.append(fn.rope_rotate(x, rot))
    return grads(outs, leaves + par)


def case_sln(C, planar):
    B, F = 5, 9
    z = rnd(B, F, C, cplx=True).requires_grad_(True)
    with torch.no_grad():
        z[0, 0, 0] = 0                                  # the m = 0 branch
    gamma, beta = (1 + 0.3 * rnd(F, C)).requires_grad_(True), (0.2 * rnd(F, C)).requires_grad_(True)
    return grads(fn.spectral_layer_norm(z, gamma, beta, 1e-5, planar=bool(planar)), [z, gamma, beta])


def case_gate(C, ref_gain):
    B, F = 3, 33
    lv = [t.requires_grad_(True) for t in (rnd(B, F, C, cplx=True), rnd(F, cplx=True), rnd(C), rnd(F).abs(),
                                           rnd(B, C).abs())]
    m = torch.ones(F, device=DEV)
    m[20:] = 0
    return grads(fn.spectral_gate(*lv, m, reference_gain_grad=bool(ref_gain)), lv)


def case_mix(n, with_c):
    lv = [t.requires_grad_(True) for t in (rnd(n), rnd(n), rnd(n))]
    c = rnd(n).requires_grad_(True) if with_c else None
    w = rnd(2).requires_grad_(True)
    return grads(fn.mix_paths(lv[0], lv[1], lv[2], c, w), lv + ([c] if with_c else []) + [w])


FAMILIES = {
    # one width per (VEC, CH) class: block VEC 4 x CH 1..16 and VEC 1 x CH 1, 4, 16
    "block": (case_block, [(D, p) for D in (256, 512, 1024, 2048, 4096, 6, 130, 518) for p in (0.0, 0.1)]),
    # enhanced VEC 4 x CH 1, 2, 4 and VEC 2 x CH 1, 2, 4, 8
    "enhanced": (case_enhanced, [(D, p) for D in (64, 256, 512, 1024, 126, 254, 510, 1022) for p in (0.0, 0.1)]),
    # spectral LN CH 1 .. 16, ragged and odd C
    "sln": (case_sln, [(C, pl) for C in (37, 64, 128, 200, 512, 1024, 999) for pl in (0, 1)]),
    "gate": (case_gate, [(C, r) for C in (512, 130, 6) for r in (0, 1)]),
    "mix": (case_mix, [(n, c) for n in (4, 1 << 20, (1 << 22) + 12) for c in (0, 1)]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="libsmx_parent.so,libsmx.so")
    ap.add_argument("--family", default=",".join(FAMILIES))
    args = ap.parse_args()
    csrc = os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc")
    names = args.libs.split(",")
    loaded = {n: _lib.load(n if os.path.isabs(n) else os.path.join(csrc, n)) for n in names}
    bad = 0
    for fam in args.family.split(","):
        run, cases = FAMILIES[fam]
        for case in cases:
            rec = {"family": fam, "case": list(case)}
            try:
                res = []
                for n in names:
                    _lib._lib = loaded[n]
                    torch.manual_seed(1000 + int(case[0]))       # same inputs and the same dropout words for every build
                    res.append([t.clone() for t in run(*case)])
                    torch.cuda.synchronize()
                rec["tensors"] = len(res[0])
                rec["equal"] = all(len(r) == len(res[0]) and all(torch.equal(bits(a), bits(b)) for a, b in zip(r, res[0]))
                                   for r in res[1:])
                rec["finite"] = all(bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all())
                                    for t in res[0])
            except Exception as e:                               # an unsupported shape is reported, not hidden
                rec["error"] = f"{type(e).__name__}: {e}"[:200]
            bad += not rec.get("equal", False)
            print(json.dumps(rec), flush=True)
            fn.release_workspaces()
    _lib._lib = loaded[names[-1]]
    print(json.dumps({"cases_differing_or_failed": bad}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
