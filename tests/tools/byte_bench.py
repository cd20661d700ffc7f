#!/usr/bin/env python3
"""Timing of the byte-spectral feature rows (functional.byte_features, smx_byte_features / smx_byte_grad_bands), forward
and forward+backward (HIP events, median of --iters eager calls; beside it the same step replayed from one hipGraph,
i.e. without the host's share).  Beside them, on the same GPU:
  * the reference's op sequence of ByteSpectralEmbedding.forward up to its projection (fft_tensor/byte_spectral_model.py:
    52-97: a Python loop over the T positions with roll, fft, abs, angle, sin, cos, cat, pad) restated in eager torch --
    a comparison point only, never part of the product, and host-bound like every eager number here;
  * a plain fill of a tensor of the output's size: the floor of a launch that has to write (B, T, W) floats;
  * freq_proj (Linear, LayerNorm, GELU, Linear) on those rows, forward: what the features feed.
Launched by hand:

    python tests/tools/byte_bench.py [--iters 50] [--shapes 64x512x256,8x512x256]
"""
import argparse, json, os, sys
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


def torch_loop(ids, bands, D):
    """the reference's per-position sequence (fft_tensor/byte_spectral_model.py:52-97) in eager torch"""
    B, T = ids.shape
    signal = (ids.float() / 127.5) - 1.0
    k = min(D // 2, T // 2)
    rows = []
    for pos in range(T):
        spectrum = torch.fft.fft(torch.roll(signal, shifts=-pos, dims=1), dim=1)
        mag = torch.abs(spectrum[:, :k]) * bands[:k]
        phase = torch.angle(spectrum[:, :k])
        f = torch.cat([mag, torch.sin(phase), torch.cos(phase)], dim=-1)
        if f.size(-1) < D:
            f = torch.cat([f, torch.zeros(B, D - f.size(-1), device=f.device)], dim=-1)
        else:
            f = f[:, :D]
        rows.append(f)
    return torch.stack(rows, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default="64x512x256,8x512x256", help="B x T x D")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for sh in args.shapes.split(","):
        B, T, D = map(int, sh.split("x"))
        ids = torch.randint(0, 256, (B, T), device=dev)
        emb = pkg.ByteSpectralEmbedding(D, T).to(dev)
        bands = emb.freq_bands
        g = torch.randn(B, T, D, device=dev)
        fill = torch.empty(B, T, D, device=dev)

        def both(make):
            def step():
                make().backward(g)
                bands.grad = None
            return step

        def fwd():
            with torch.no_grad():
                return pkg.byte_features(ids, bands, D, native=True)
        ours = both(lambda: pkg.byte_features(ids, bands, D, native=True))
        rec = {"op": "byte_features", "shape": sh, "out_MiB": round(B * T * D * 4 / 2 ** 20, 1),
               "fwd_ms": round(timeit(fwd, args.iters), 4), "fwd_graph_ms": round(graphed(fwd, args.iters), 4),
               "fwd_bwd_ms": round(timeit(ours, args.iters), 4), "fwd_bwd_graph_ms": round(graphed(ours, args.iters), 4),
               "fill_ms": round(timeit(lambda: fill.fill_(1.0), args.iters), 4),
               "fill_graph_ms": round(graphed(lambda: fill.fill_(1.0), args.iters), 4)}
        feats = fwd()

        def proj():
            with torch.no_grad():
                return emb.freq_proj(feats)
        rec["freq_proj_fwd_ms"] = round(timeit(proj, args.iters), 4)
        rec["freq_proj_fwd_graph_ms"] = round(graphed(proj, args.iters), 4)
        if not args.no_torch:
            few = max(3, args.iters // 16)

            def loop_fwd():
                with torch.no_grad():
                    return torch_loop(ids, bands, D)
            rec["torch_position_loop_fwd_ms"] = round(timeit(loop_fwd, few, warm=1), 2)
            rec["torch_position_loop_fwd_bwd_ms"] = round(timeit(both(lambda: torch_loop(ids, bands, D)), few, warm=1), 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
