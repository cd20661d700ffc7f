#!/usr/bin/env python3
"""Timing of the SpectralEMA scan, forward+backward (HIP events, median of --iters eager calls; beside it the same
step replayed from one hipGraph, i.e. without the host's share): the reference's op sequence in eager torch on the
same GPU (a comparison point only, never part of the product), functional.ema_scan on the chunk spectra, and
functional.ema_scan_tokens on the byte tokens themselves (chunk_len 2 (F - 1); not run for the wide case, whose
chunk length is past the front end's 64).  Launched by hand:

    python tests/tools/ema_bench.py [--iters 50] [--shapes 8x64x9,64x64x9,64x64x513]
"""
import argparse, json, math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import tensor_cuda_fft_amd as pkg


def timeit(f, iters, warm=3):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    evs = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); evs.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2]


def graphed(step, iters, n=10):
    """ms per step with n steps replayed from one hipGraph"""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        step(); step()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(n):
            step()
    return timeit(gr.replay, iters) / n


def torch_scan(chunks, rl, tr, mode):
    """the reference's per-step sequence (fft_lm/spectral_ssm.py:71-125) in eager torch"""
    rho = torch.sigmoid(rl)
    keep = 1.0 - rho
    a = (rho * torch.exp(1j * (math.pi * torch.tanh(tr)))).to(torch.complex64)
    state = torch.zeros(chunks.shape[0], chunks.shape[2], dtype=torch.complex64, device=chunks.device)
    for t in range(chunks.shape[1]):
        x = chunks[:, t]
        if mode == "polar":
            mag = rho[None] * state.abs() + keep[None] * x.abs()
            state = mag.to(torch.complex64) * torch.exp(1j * x.angle())
        else:
            state = a[None] * (state * torch.exp(1j * (x.angle() - state.angle()))) + keep[None] * x
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default="8x64x9,64x64x9,64x64x513", help="B x S x F")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for sh in args.shapes.split(","):
        B, S, F = map(int, sh.split("x"))
        L = 2 * (F - 1)
        for mode in (("aligned", "polar") if F < 100 else ("aligned",)):
            rl = (2.0 + torch.randn(F, device=dev)).requires_grad_(True)
            tr = (0.5 * torch.randn(F, device=dev)).requires_grad_(True)
            g = torch.randn(B, F, dtype=torch.complex64, device=dev)
            tokens = torch.randint(0, 256, (B, S * L), device=dev) if L <= 64 else None
            if tokens is not None:
                chunks = torch.fft.rfft(tokens.reshape(B, S, L).float() / 127.5 - 1.0, dim=-1)
            else:
                chunks = torch.randn(B, S, F, dtype=torch.complex64, device=dev)

            def run(scan):
                def step():
                    scan().backward(g)
                    rl.grad = tr.grad = None
                return step
            ours = run(lambda: pkg.ema_scan(chunks, rl, tr, mode))
            rec = {"op": "SpectralEMA scan fwd+bwd", "shape": sh, "mode": mode,
                   "ema_scan_ms": round(timeit(ours, args.iters), 4), "ema_scan_graph_ms": round(graphed(ours, args.iters), 4)}
            if tokens is not None:
                toks = run(lambda: pkg.ema_scan_tokens(tokens, L, rl, tr, mode))
                rec["ema_scan_tokens_ms"] = round(timeit(toks, args.iters), 4)
                rec["ema_scan_tokens_graph_ms"] = round(graphed(toks, args.iters), 4)
            if not args.no_torch:
                rec["torch_loop_ms"] = round(timeit(run(lambda: torch_scan(chunks, rl, tr, mode)), max(5, args.iters // 5)), 4)
                rec["torch_over_ema_scan"] = round(rec["torch_loop_ms"] / rec["ema_scan_ms"], 1)
                if tokens is not None:
                    rec["torch_over_ema_scan_tokens"] = round(rec["torch_loop_ms"] / rec["ema_scan_tokens_ms"], 1)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
