#!/usr/bin/env python3
"""Timing of the native FFT convolutions (optimized_ops.fast_frequency_conv1d / conv2d on functional.bin_contract,
csrc/smx_fconv.hip) beside the reference's own op sequence through torch.fft on the same GPU (restated here:
fft_tensor/optimized_ops.py:166-200, :229-265), beside F.conv1d / F.conv2d of the same operands (a yardstick of cost
only: they compute a cross-correlation, another result) and, for the contraction alone, beside a device copy of the bytes
it has to move.  Launched by hand, not a pass/fail test:

    python tests/tools/optops_bench.py [--cases conv1d:8x64x64x4096x1024,conv1d:8x64x64x1024x128,conv2d:4x16x16x128x128x31x31]
                                       [--out profiles/optops_bench.txt]

Every case runs in a child process of its own under its own time limit; the first that fails, faults or runs out of time
ends the run (nothing more is started on the GPU after it).  One JSON line per case.  HIP events around each eager call,
the candidates alternating within one loop; median, minimum and count are printed.
Bytes of the contraction, counted from the shapes: x (B P Ci) and w (P Ci Co) read once, y (B P Co) written once, 8 bytes
each; the copy yardstick moves exactly that many bytes with Tensor.copy_ (half read, half written)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMIT = 300                                                   # seconds per child


def events_ms(f):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "runs": len(ts)}


def race(fns, runs):
    """{name: stats}: the candidates alternate inside each round"""
    for f in fns.values():
        f(); f()
    ts = {n: [] for n in fns}
    for _ in range(runs):
        for n, f in fns.items():
            ts[n].append(events_ms(f))
    return {n: stats(v) for n, v in ts.items()}


def next_pow2(n):
    import numpy as np
    return 2 ** int(np.ceil(np.log2(n)))


def reference_conv1d(x, w):
    import torch
    import torch.nn.functional as F
    L, K = x.shape[-1], w.shape[-1]
    n = next_pow2(L + K - 1)
    xf = torch.fft.fft(F.pad(x, (0, n - L)), dim=-1)
    wf = torch.fft.fft(F.pad(w, (0, n - K)), dim=-1)
    return torch.fft.ifft((xf.unsqueeze(1) * wf.unsqueeze(0)).sum(dim=2), dim=-1).real[:, :, :L - K + 1]


def reference_conv2d(x, w):
    import torch
    import torch.nn.functional as F
    (H, W), (Kh, Kw) = x.shape[-2:], w.shape[-2:]
    nh, nw = next_pow2(H + Kh - 1), next_pow2(W + Kw - 1)
    xf = torch.fft.fft2(F.pad(x, (0, nw - W, 0, nh - H)), dim=(-2, -1))
    wf = torch.fft.fft2(F.pad(w, (0, nw - Kw, 0, nh - Kh)), dim=(-2, -1))
    return torch.fft.ifft2((xf.unsqueeze(1) * wf.unsqueeze(0)).sum(dim=2), dim=(-2, -1)).real[:, :, :H - Kh + 1, :W - Kw + 1]


def step(case):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import functional as fn
    O = pkg.OptimizedFrequencyOps
    kind, _, dims = case.partition(":")
    dims = tuple(int(v) for v in dims.split("x"))
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1234)
    rec = {"step": case}
    if kind == "conv1d":
        B, Ci, Co, L, K = dims
        x = torch.randn(B, Ci, L, device=dev, generator=gen)
        w = torch.randn(Co, Ci, K, device=dev, generator=gen) / (Ci * K) ** 0.5
        native, reference, direct = O.fast_frequency_conv1d, reference_conv1d, F.conv1d
        P = next_pow2(L + K - 1) // 2 + 1
        rec["reference_intermediate_bytes"] = 8 * B * Co * Ci * next_pow2(L + K - 1)
    elif kind == "conv2d":
        B, Ci, Co, H, W, Kh, Kw = dims
        x = torch.randn(B, Ci, H, W, device=dev, generator=gen)
        w = torch.randn(Co, Ci, Kh, Kw, device=dev, generator=gen) / (Ci * Kh * Kw) ** 0.5
        native, reference, direct = O.fast_frequency_conv2d, reference_conv2d, F.conv2d
        P = (next_pow2(H + Kh - 1) // 2 + 1) * next_pow2(W + Kw - 1)
        rec["reference_intermediate_bytes"] = 8 * B * Co * Ci * next_pow2(H + Kh - 1) * next_pow2(W + Kw - 1)
    else:
        sys.exit(f"unknown case {case!r}")
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    with torch.no_grad():
        got, want = native(x, w), reference(x, w)
        rec["max_normalised_difference"] = float((got - want).abs().max() / want.abs().max())
        g = torch.randn(got.shape, device=dev, generator=gen)
        del got, want

    def fwd_bwd():
        return torch.autograd.grad(native(xg, wg), (xg, wg), g)

    def crandn(*shape):
        return torch.complex(torch.randn(*shape, device=dev, generator=gen), torch.randn(*shape, device=dev, generator=gen))
    xs, ws = crandn(B, P, Ci), crandn(P, Ci, Co)
    xsg, wsg, gy = xs.clone().requires_grad_(), ws.clone().requires_grad_(), crandn(B, P, Co)
    nbytes = 8 * (B * P * Ci + P * Ci * Co + B * P * Co)
    src, dst = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    rec["bins"], rec["bin_contract_bytes"] = P, nbytes
    with torch.no_grad():
        r = race({"native_forward": lambda: native(x, w), "reference_ops_torch_fft": lambda: reference(x, w),
                  "bin_contract": lambda: fn.bin_contract(xs, ws),
                  "einsum": lambda: torch.einsum("bpi,pio->bpo", xs, ws), "copy_same_bytes": lambda: dst.copy_(src)}, 20)
        r.update(race({"direct_conv": lambda: direct(x, w)}, 5))          # (can be slow at these kernel sizes: five runs)
    r.update(race({"native_forward_backward": fwd_bwd,
                   "bin_contract_forward_backward": lambda: torch.autograd.grad(fn.bin_contract(xsg, wsg), (xsg, wsg), gy)}, 20))
    rec.update(r)
    rec["bin_contract"]["GBps"] = round(nbytes / r["bin_contract"]["median_ms"] / 1e6, 1)
    rec["copy_same_bytes"]["GBps"] = round(nbytes / r["copy_same_bytes"]["median_ms"] / 1e6, 1)
    rec["reference_over_native"] = round(r["reference_ops_torch_fft"]["median_ms"] / r["native_forward"]["median_ms"], 2)
    rec["direct_over_native"] = round(r["direct_conv"]["median_ms"] / r["native_forward"]["median_ms"], 2)
    rec["bin_contract_over_copy"] = round(r["bin_contract"]["median_ms"] / r["copy_same_bytes"]["median_ms"], 2)
    rec["einsum_over_bin_contract"] = round(r["einsum"]["median_ms"] / r["bin_contract"]["median_ms"], 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="conv1d:8x64x64x4096x1024,conv1d:8x64x64x1024x128,conv2d:4x16x16x128x128x31x31")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return step(args.child)
    lines = []
    for case in filter(None, args.cases.split(",")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], capture_output=True, text=True,
                               timeout=LIMIT)
        except subprocess.TimeoutExpired:
            sys.exit(f"{case}: no result within its time limit; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"{case}: exit status {r.returncode}; nothing more is started\n{r.stderr[-3000:]}")
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        print("\n".join(out), flush=True)
        lines += out
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
