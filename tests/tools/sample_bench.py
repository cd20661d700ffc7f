#!/usr/bin/env python3
"""Timing of the native byte sampler (functional.sample_bytes, smx_sample_bytes) and of chunk generation with it.

  a) the sampler alone on (16, 256) and (1, 256) logits with a 256-id window, temperature 0.9, top_p 0.9, repetition
     penalty 1.15 (generate_chunked's defaults): `native` = torch.rand + sample_bytes, beside `torch_chunk` =
     streaming._sample_chunk, the eager-torch sampler generate_chunked(sampler="torch") runs (about a dozen small ops and
     torch.multinomial).  Each eager (HIP events around one call, host-bound), median of --iters; the native one also
     replayed from one hipGraph (the device time alone).  The torch sampler cannot be captured -- its `seen[recent] = True`
     is refused while a stream is capturing -- so it has no graph figure: eager is the only way it runs.
  b) `reference_loop`: the reference's per-row sampler (scripts/stream_generate_fast.py:146-170: a Python loop over
     set(recent) with one indexed division each, sort / softmax / cumsum, `.item()` for the cut and `.item()` after
     multinomial) restated with torch on the same GPU and run row by row -- eager only, it synchronises the host; a
     comparison point, never part of the product.
  c) one whole generated chunk at fft_lm's generation shape (seq_len 1024, kernel_len 128, d_model 512, 6 layers,
     chunk 16, EMA memory on): generate_chunked(..., use_graph=True) with sampler="torch" beside sampler="native", as
     wall-clock time per chunk = (t(--long chunks) - t(--short chunks)) / (long - short), the two alternating over
     --rounds rounds, median.

Launched by hand:

    python tests/tools/sample_bench.py [--iters 50] [--rounds 5] [--short 8] [--long 72]
"""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import tensor_cuda_fft_amd as pkg
from tensor_cuda_fft_amd.streaming import _sample_chunk
from ema_bench import timeit, graphed

TEMPERATURE, TOP_P, REP = 0.9, 0.9, 1.15


def reference_loop(logits, recent_list):
    """the reference's sample_next, one row at a time"""
    out = []
    for row in logits:
        l = row.float().clone()
        for tok in set(recent_list[-256:]):
            l[tok] = l[tok] / REP
        l = l / TEMPERATURE
        sl, si = torch.sort(l, descending=True)
        keep = torch.cumsum(torch.softmax(sl, dim=-1), dim=-1) <= TOP_P
        keep[0] = True
        cut = int(keep.sum().item())
        masked = torch.full_like(l, -float("inf"))
        masked[si[:cut]] = l[si[:cut]]
        out.append(int(torch.multinomial(torch.softmax(masked, dim=-1), 1).item()))
    return out


def sampler_alone(dev, rows, iters):
    logits = 3.0 * torch.randn(rows, 256, device=dev)
    recent = torch.randint(97, 123, (256,), device=dev)
    recent_list = recent.tolist()

    def native():
        u = torch.rand(rows, device=dev)
        return pkg.sample_bytes(logits, recent, u, temperature=TEMPERATURE, top_p=TOP_P, repetition_penalty=REP)

    torch_chunk = lambda: _sample_chunk(logits, recent, TEMPERATURE, TOP_P, REP, None)
    rec = {"op": "sampler alone", "rows": rows, "n_recent": 256, "iters": iters,
           "native_eager_ms": round(timeit(native, iters), 4), "native_graph_ms": round(graphed(native, iters), 4),
           "torch_chunk_eager_ms": round(timeit(torch_chunk, iters), 4), "torch_chunk_graph_ms": None,
           "reference_loop_eager_ms": round(timeit(lambda: reference_loop(logits, recent_list), max(iters // 5, 5)), 4)}
    rec["torch_chunk_over_native_eager"] = round(rec["torch_chunk_eager_ms"] / rec["native_eager_ms"], 2)
    rec["reference_loop_over_native_eager"] = round(rec["reference_loop_eager_ms"] / rec["native_eager_ms"], 2)
    print(json.dumps(rec), flush=True)


def whole_chunk(dev, rounds, short, long):
    cfg, chunk = pkg.LMConfig(), 16
    torch.manual_seed(0)
    model = pkg.ChunkLM(pkg.FixedSpectralLM(cfg), chunk, use_ema=True, ema_chunk_len=16).to(dev).eval()
    with torch.no_grad():
        model.head.weight.normal_(0.0, 0.05)
        for blk in model.backbone.blocks:
            blk.kernel.normal_(0.0, 0.3)

    def wall(sampler, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pkg.generate_chunked(model, b"Once upon a time", n, sampler=sampler, use_graph=True)
        assert len(out) == cfg.seq_len + n * chunk
        return (time.perf_counter() - t0) * 1e3

    ms = {"torch": [], "native": []}
    for s in ms:
        wall(s, short)                                                    # warm-up
    for _ in range(rounds):
        for s in ms:
            a, b = wall(s, short), wall(s, long)
            ms[s].append((b - a) / (long - short))
    rec = {"op": "generate_chunked per chunk, use_graph=True", "seq_len": cfg.seq_len, "kernel_len": cfg.kernel_len,
           "d_model": cfg.d_model, "layers": cfg.n_layers, "chunk": chunk, "rounds": rounds, "chunks": [short, long]}
    for s, v in ms.items():
        v = sorted(v)
        rec[f"sampler_{s}_ms"] = round(v[len(v) // 2], 4)
        rec[f"sampler_{s}_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
    rec["torch_over_native"] = round(rec["sampler_torch_ms"] / rec["sampler_native_ms"], 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=72)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for rows in (16, 1):
        sampler_alone(dev, rows, args.iters)
    whole_chunk(dev, args.rounds, args.short, args.long)


if __name__ == "__main__":
    main()
