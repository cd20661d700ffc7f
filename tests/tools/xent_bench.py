#!/usr/bin/env python3
"""Timing of the native cross-entropy (HIP events, median of --iters calls after warm-up; beside the eager figure the same
step replayed from one hipGraph, i.e. without the host's share):

  * functional.cross_entropy forward + backward (mean reduction) beside nn.functional.cross_entropy on the same GPU and the
    same tensors, at the dual head's token loss (8192, 50257) with ignore_index = 0, at (8192, 4096) and at the char loss
    (128, 256).  The two results (loss and gradient) are compared before anything is printed.
  * hbm_fraction: 3 R V 4 bytes (one read forward, one read and one write backward) in the graph-replay time, over 8 TB/s.

Launched by hand:

    python tests/tools/xent_bench.py [--iters 30] [--shapes 8192x50257,8192x4096,128x256]
"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import tensor_cuda_fft_amd as pkg
from ema_bench import timeit, graphed

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--shapes", default="8192x50257,8192x4096,128x256", help="R x V")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for sh in args.shapes.split(","):
        R, V = map(int, sh.split("x"))
        ignore = 0 if V == 50257 else -100
        x = (2.0 * torch.randn(R, V, device=dev)).requires_grad_(True)
        y = torch.randint(0, V, (R,), device=dev)

        def run(op):
            def step():
                op(x, y, ignore_index=ignore).backward()
                x.grad = None
            return step

        def result(op):
            loss = op(x, y, ignore_index=ignore)
            (grad,) = torch.autograd.grad(loss, x)
            return loss.detach(), grad

        (l0, g0), (l1, g1) = result(pkg.cross_entropy), result(torch.nn.functional.cross_entropy)
        err_loss = float((l0 - l1).abs() / l1.abs())
        err_grad = float((g0 - g1).abs().max() / g1.abs().max())
        assert err_loss <= 1e-5 and err_grad <= 1e-5, (sh, err_loss, err_grad)
        del g0, g1
        ours, ref = run(pkg.cross_entropy), run(torch.nn.functional.cross_entropy)
        n = 10 if R * V < (1 << 26) else 2
        rec = {"op": "cross_entropy fwd+bwd (mean)", "rows": R, "V": V, "ignore_index": ignore,
               "err_loss_vs_torch": float("%.1e" % err_loss), "err_grad_vs_torch": float("%.1e" % err_grad),
               "native_ms": round(timeit(ours, args.iters), 4), "native_graph_ms": round(graphed(ours, args.iters, n), 4),
               "torch_ms": round(timeit(ref, args.iters), 4), "torch_graph_ms": round(graphed(ref, args.iters, n), 4)}
        rec["torch_over_native_graph"] = round(rec["torch_graph_ms"] / rec["native_graph_ms"], 2)
        rec["hbm_fraction"] = round(3.0 * R * V * 4 / (rec["native_graph_ms"] * 1e-3) / HBM_BYTES_PER_S, 3)
        print(json.dumps(rec), flush=True)
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
