#!/usr/bin/env python3
"""Timing of the word-structure heads (HIP events, median of --iters calls after warm-up; beside the eager figure the same
step replayed from one hipGraph, i.e. without the host's share):

  * functional.word_targets (both outputs, one launch) beside the reference's two target functions restated op for op in
    eager torch ON THE SAME DEVICE TENSOR -- the per-byte `.item()` walk of fft_lm/phase_clock.py:83-113 (wall clock, it
    synchronises the host at every byte; timed once, at the first shape only) and the per-position loop of
    fft_lm/segmentation_head.py:77-97.  Comparison points only, never part of the product;
  * functional.narrow_head forward+backward (grad_h, grad_w, grad_b) beside F.linear, O = 1 and 2, over B T rows of width C.

Launched by hand:

    python tests/tools/heads_bench.py [--iters 50] [--shapes 8x1024,64x1024] [--width 512]
"""
import argparse, json, math, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import tensor_cuda_fft_amd as pkg
from ema_bench import timeit, graphed


def item_walk_phase(x):
    """generate_phase_targets as the reference walks it: one host read per byte, one linspace / cos / sin per word"""
    B, T = x.shape
    brk = lambda v: v == 32 or 33 <= v <= 47 or 58 <= v <= 64
    out = torch.zeros(B, T, 2)
    for b in range(B):
        i = 0
        while i < T:
            if brk(x[b, i].item()):
                i += 1
                continue
            j = i
            while j < T and not brk(x[b, j].item()):
                j += 1
            ang = torch.linspace(0, math.pi, j - i)
            out[b, i:j, 0] = torch.cos(ang)
            out[b, i:j, 1] = torch.sin(ang)
            i = j
    return out


def position_loop_boundaries(x):
    """get_word_boundaries as the reference loops it: about fourteen elementwise launches per position"""
    out = torch.zeros_like(x, dtype=torch.float32)
    for t in range(x.shape[1] - 1):
        n = x[:, t + 1]
        hit = (n == 32) | ((n >= 33) & (n <= 47)) | ((n >= 58) & (n <= 64)) | ((n >= 91) & (n <= 96)) \
            | ((n >= 123) & (n <= 126)) | (n == 10) | (n == 13)
        out[:, t] = hit.float()
    out[:, -1] = 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default="8x1024,64x1024", help="B x T")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    C = args.width
    text = torch.tensor(list(b"the quick brown fox, jumps over {the} lazy dog.\n"), dtype=torch.int64)
    for n_shape, sh in enumerate(args.shapes.split(",")):
        B, T = map(int, sh.split("x"))
        x = text.repeat(B * T // len(text) + 1)[:B * T].reshape(B, T).to(dev)
        rec = {"op": "word_targets (phase + boundary)", "shape": sh}
        for name, tok in (("int64", x), ("uint8", x.to(torch.uint8))):
            step = lambda tok=tok: pkg.word_targets(tok)
            rec[f"word_targets_{name}_ms"] = round(timeit(step, args.iters), 4)
            rec[f"word_targets_{name}_graph_ms"] = round(graphed(step, args.iters), 4)
        if not args.no_torch:
            rec["torch_position_loop_boundaries_ms"] = round(timeit(lambda: position_loop_boundaries(x), 3, warm=1), 2)
            if n_shape == 0:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                item_walk_phase(x)
                rec["torch_item_walk_phase_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        print(json.dumps(rec), flush=True)
        for O in (1, 2):
            h = torch.randn(B, T, C, device=dev, requires_grad=True)
            w = (0.1 * torch.randn(O, C, device=dev)).requires_grad_(True)
            b = torch.zeros(O, device=dev, requires_grad=True)
            g = torch.randn(B, T, O, device=dev)

            def run(op):
                def step():
                    op(h, w, b).backward(g)
                    h.grad = w.grad = b.grad = None
                return step
            ours, lin = run(pkg.narrow_head), run(torch.nn.functional.linear)
            rec = {"op": "narrow_head fwd+bwd", "rows": B * T, "C": C, "O": O,
                   "narrow_head_ms": round(timeit(ours, args.iters), 4),
                   "narrow_head_graph_ms": round(graphed(ours, args.iters), 4),
                   "linear_ms": round(timeit(lin, args.iters), 4), "linear_graph_ms": round(graphed(lin, args.iters), 4)}
            rec["linear_over_narrow_head_graph"] = round(rec["linear_graph_ms"] / rec["narrow_head_graph_ms"], 2)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
