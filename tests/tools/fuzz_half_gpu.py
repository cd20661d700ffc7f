#!/usr/bin/env python3
"""Random shapes across every plan in bf16 and fp16 against the bitwise contract of the 2-byte activations:

    y == layer_fp32(x.float()).to(dtype), grad_x == ....to(dtype), parameter gradients == the fp32 path's

with training-mode fused dropout on half of the cases (the same DropoutState words for both calls).

    python tests/tools/fuzz_half_gpu.py --cases 2000 [--seed 0] [--out profiles/r05_half_fuzz.txt]
"""
import argparse
import collections
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import tensor_cuda_fft_amd as pkg  # noqa: E402
from tensor_cuda_fft_amd import _lib  # noqa: E402


def bits(t):
    t = t.masked_fill(torch.isnan(t), 0)
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return bool(torch.equal(torch.isnan(a), torch.isnan(b))) and bool(torch.equal(bits(a), bits(b)))


def shape(rng):
    kind = rng.choice(["fused", "fused", "split", "direct", "sixteen", "over512", "oddD"])
    if kind in ("fused", "split"):
        N = 256 * rng.choice([1, 2, 4, 8, 16] if kind == "fused" else [16, 32, 64])
        D = 2 * rng.randint(1, 80)
        F = rng.choice([rng.randint(1, 128), rng.randint(129, 256), rng.randint(257, 512)])
        B = rng.randint(1, 16) if kind == "fused" else rng.randint(1, 3)
    elif kind == "direct":
        N, D, F, B = rng.randint(2, 1500), 2 * rng.randint(1, 16), rng.randint(1, 64), rng.randint(1, 4)
    elif kind == "sixteen":
        N, D, F, B = 16 * rng.choice([17, 31, 65, 100]), 2 * rng.randint(1, 24), rng.randint(1, 128), rng.randint(1, 4)
    elif kind == "over512":
        N, D, F, B = 256 * rng.choice([5, 8, 16]), 2 * rng.randint(1, 8), rng.randint(513, 1200), rng.randint(1, 2)
    else:
        N, D, F, B = 256 * rng.randint(1, 8), 2 * rng.randint(1, 16) + 1, rng.randint(1, 200), rng.randint(1, 4)
    return B, N, D, F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = random.Random(a.seed)
    tally = collections.Counter()
    fails = []
    t0 = time.time()
    for i in range(a.cases):
        B, N, D, F = shape(rng)
        dtype = rng.choice([torch.bfloat16, torch.float16])
        drop = rng.random() < 0.5
        p = _lib.plan(B, N, D, F)
        io = 1 if dtype == torch.bfloat16 else 2
        native = _lib.io_supported(B, N, D, F, io)
        key = ("native" if native else "upcast") + ("/split" if native and p.nsplit > 1 else "") + \
            (f"/nb{p.bands}" if native else f"/path{p.path}") + ("/drop" if drop else "")
        torch.manual_seed(i)
        layer = pkg.SpectralMixingLayer(D, num_filters=F, dropout=0.2 if drop else 0.0).to(dev)
        with torch.no_grad():
            layer.weight_real.normal_(1.0, 0.5); layer.weight_imag.normal_(0.0, 0.5); layer.bias.normal_(0.0, 0.1)
        layer.train(drop)
        x = torch.randn(B, N, D, device=dev).to(dtype)
        g = torch.randn(B, N, D, device=dev).to(dtype)
        outs = []
        for xin, gin in ((x, g), (x.float(), g.float())):
            xr = xin.clone().requires_grad_(True)
            for q in layer.parameters():
                q.grad = None
            torch.manual_seed(10_000 + i)
            y = layer(xr)
            y.backward(gin)
            outs.append([y.detach(), xr.grad, layer.weight_real.grad.clone(), layer.weight_imag.grad.clone(),
                         layer.bias.grad.clone()])
        h, f = outs
        ok = same(h[0], f[0].to(dtype)) and same(h[1], f[1].to(dtype)) and all(same(u, v) for u, v in zip(h[2:], f[2:]))
        tally[key] += 1
        if not ok:
            fails.append((i, (B, N, D, F), str(dtype), drop, key))
    torch.cuda.synchronize()
    lines = [f"fuzz_half_gpu: {a.cases} cases, seed {a.seed}, {len(fails)} failures, {time.time() - t0:.0f} s",
             "cases by route (native = IO instances of k_fused / k_split_*, upcast = fp32 op + .to(dtype)):"]
    lines += [f"  {k:28s} {v}" for k, v in sorted(tally.items())]
    lines += [f"  FAIL case {c}: shape {s} {d} dropout={dr} {k}" for c, s, d, dr, k in fails[:50]]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
