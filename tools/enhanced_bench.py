#!/usr/bin/env python3
"""fwd+bwd of EnhancedSpectralBlock (reference fft_tensor/spectral_enhancements.py:278-333): the fused row kernels
(fuse_rows = True) against the reference's op sequence on the same native transforms (fuse_rows = False), timed with
device events in one process, the two variants alternated round by round.  Workloads:
  stack  benchmark_enhanced.py's model body: 4 x EnhancedSpectralBlock(256) at (4, 512, 256), eager and in a hipGraph
  big    one block at (64, 4096, 256), eager
Prints one JSON line: ms per fwd+bwd (median over rounds) and the algorithmic bytes per (b, t, d) sample of each row
line, fused kernels and the torch composition they replace.  Achieved bandwidth = bytes x samples / kernel time, the
kernel time from a rocprofv3 --kernel-trace --stats run of this tool (--only big --rounds 3).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensor_cuda_fft_amd as pkg  # noqa: E402

# bytes per sample (fp32, eval mode).  Fused: what each kernel reads and writes (A/B/C of csrc/smx_enh.hip; the gate
# row a is 2D wide).  Composition: the sum over the torch ops of the same line of their inputs read and outputs
# written (complex views and chunks are free; the rotation table and LayerNorm statistics are per row, not counted).
BYTES = {
    "fused": {
        "A_rope_norm": {"fwd": 4 + 8, "bwd": 12 + 4},         # x -> x1, h2 | g1, gh2, x -> grad_x
        "B_residual_norm": {"fwd": 8 + 8, "bwd": 12 + 4},     # x1, p -> x2, h3 | g2, gh3, x2 -> grad_x1
        "C_gate_blend": {"fwd": 16 + 4, "bwd": 16 + 12},      # a, v, x2 -> x3 | g3, a, v -> grad_a, grad_v
    },
    "composition": {
        # norm1 8, complex() 8, rotation product 8, stack 8, residual add 12, norm2 8
        "A_rope_norm": {"fwd": 52},
        # residual add 12, norm3 8
        "B_residual_norm": {"fwd": 20},
        # LayerNorm(2D) 16, sigmoid 8, gate*v 12, 1-gate 8, (1-gate)*vt 12, sum 12, residual add 12
        "C_gate_blend": {"fwd": 80},
    },
}


def timed(step, rounds, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        step()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def make(D, n, dev):
    torch.manual_seed(0)
    blocks = torch.nn.ModuleList([pkg.EnhancedSpectralBlock(D) for _ in range(n)]).to(dev).eval()
    with torch.no_grad():
        for p in blocks.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return blocks


def runner(blocks, x, g):
    def step():
        for p in blocks.parameters():
            p.grad = None
        x.grad = None
        y = x
        for b in blocks:
            y = b(y)
        y.backward(g)
    return step


def graphed(step, dev):
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step()
    return gr.replay


def set_fused(blocks, on):
    for b in blocks:
        b.fuse_rows = on


def bench(name, blocks, B, T, D, dev, rounds, iters, graph):
    x = torch.randn(B, T, D, device=dev, requires_grad=True)
    g = torch.randn(B, T, D, device=dev)
    step = runner(blocks, x, g)
    fns = {}
    for variant, on in (("fused", True), ("composition", False)):
        set_fused(blocks, on)
        for _ in range(3):
            step()
        fns[variant] = graphed(step, dev) if graph else step
    times = {"fused": [], "composition": []}
    for _ in range(rounds):
        for variant in ("fused", "composition"):
            set_fused(blocks, variant == "fused")
            times[variant].append(timed(fns[variant], rounds, iters))
    set_fused(blocks, True)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"workload": name, "shape": [B, T, D], "blocks": len(blocks), "graph": graph,
            "ms_fused": round(med["fused"], 4), "ms_composition": round(med["composition"], 4),
            "speedup": round(med["composition"] / med["fused"], 3),
            "ms_fused_all": [round(t, 4) for t in times["fused"]],
            "ms_composition_all": [round(t, 4) for t in times["composition"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="", help="stack | big")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": "enhanced_bench", "bytes_per_sample": BYTES, "results": []}
    if args.only in ("", "stack"):
        stack = make(256, 4, dev)
        out["results"].append(bench("stack_eager", stack, 4, 512, 256, dev, args.rounds, args.iters, False))
        out["results"].append(bench("stack_graph", stack, 4, 512, 256, dev, args.rounds, args.iters, True))
        del stack
    if args.only in ("", "big"):
        big = make(256, 1, dev)
        out["results"].append(bench("big_eager", big, 64, 4096, 256, dev, args.rounds, max(1, args.iters // 5),
                                    False))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
