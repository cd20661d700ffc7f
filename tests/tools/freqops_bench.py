#!/usr/bin/env python3
"""Timing of the native frequency attention and frequency layernorm (csrc/smx_freq.hip) and of FrequencyTransformerLayer
beside the reference's op sequences in eager torch on the same GPU (restated here: fft_tensor/frequency_ops.py:166-185,
:342-363, :390-401) and beside a plain copy of the same number of bytes.  Launched by hand, not a pass/fail test:

    python tests/tools/freqops_bench.py [--cases attn:8x8x4096x64,attn:8x8x512x64,ln:64x4096x256,layer:8x1024x512x8]
                                        [--out profiles/freqops_bench.txt]

Every case runs in a child process of its own under its own time limit; the first that fails, faults or runs out of time
ends the run (nothing more is started on the GPU after it).  One JSON line per case.  HIP events around each call, the
native op and its yardsticks alternating within one loop; median, minimum and count are printed.  "eager": one call per
event pair, host cost included.  "graph": ten calls captured in one hipGraph, the replay timed, per call.
Bytes are counted from the shapes: the attention needs q and k once, v once and writes out once = 32 bytes per complex
element (the scores are 4 bytes per ROW); the layernorm reads and writes a row once = 16 bytes per element.  The copy
yardstick moves exactly that many bytes with Tensor.copy_.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMIT = 300                                                   # seconds per child
GRAPH_CALLS = 10


def events_ms(f):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "runs": len(ts)}


def graphed(f):
    """a replayable graph of GRAPH_CALLS calls of f (f ran eagerly before)"""
    import torch
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        f(); f()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            f()
    return g


def race(fns, runs):
    """{name: {"eager": stats, "graph": stats}}: the candidates alternate inside each round"""
    for f in fns.values():
        f(); f()
    graphs = {n: graphed(f) for n, f in fns.items()}
    for g in graphs.values():
        g.replay()
    eager, graph = {n: [] for n in fns}, {n: [] for n in fns}
    for _ in range(runs):
        for n, f in fns.items():
            eager[n].append(events_ms(f))
        for n, g in graphs.items():
            graph[n].append(events_ms(g.replay) / GRAPH_CALLS)
    return {n: {"eager": stats(eager[n]), "graph": stats(graph[n])} for n in fns}


def reference_attention(q, k, v, temperature=1.0):
    import torch
    scores = (torch.abs(q * torch.conj(k)) / temperature).mean(dim=-1)
    return torch.softmax(scores, dim=-1).unsqueeze(-1) * v


def reference_layernorm(z, eps=1e-5):
    import torch
    m = torch.abs(z)
    return (m - m.mean(dim=-1, keepdim=True)) / (m.std(dim=-1, keepdim=True) + eps) * torch.exp(1j * torch.angle(z))


def rates(rec, names, nbytes):
    for n in names:
        for mode in ("eager", "graph"):
            rec[n][mode]["GBps"] = round(nbytes / rec[n][mode]["median_ms"] / 1e6, 1)


def step(case):
    import torch
    sys.path.insert(0, ROOT)
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import functional as fn
    kind, _, dims = case.partition(":")
    dims = tuple(int(v) for v in dims.split("x"))
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1234)

    def crandn(*shape):
        return torch.complex(torch.randn(*shape, device=dev, generator=gen), torch.randn(*shape, device=dev, generator=gen))
    rec = {"step": case}
    if kind == "attn":
        q, k, v = crandn(*dims), crandn(*dims), crandn(*dims)
        n = q.numel()
        src, dst = torch.empty(2 * n, dtype=torch.complex64, device=dev), torch.empty(2 * n, dtype=torch.complex64, device=dev)
        with torch.no_grad():
            got, want = fn.frequency_attention(q, k, v), reference_attention(q, k, v)
            rec["max_normalised_difference"] = float((got - want).abs().max() / want.abs().max())
            del got, want
            r = race({"native": lambda: fn.frequency_attention(q, k, v), "reference_ops": lambda: reference_attention(q, k, v),
                      "copy_32B_per_element": lambda: dst.copy_(src)}, 20)
        rec.update(r)
        rec["bytes_needed"] = 32 * n + 8 * (n // dims[-1])
        rates(rec, r, rec["bytes_needed"])
        for mode in ("eager", "graph"):
            rec[f"reference_over_native_{mode}"] = round(r["reference_ops"][mode]["median_ms"] / r["native"][mode]["median_ms"], 2)
            rec[f"native_over_copy_{mode}"] = round(r["native"][mode]["median_ms"] / r["copy_32B_per_element"][mode]["median_ms"], 2)
    elif kind == "ln":
        z = crandn(*dims)
        n = z.numel()
        dst = torch.empty_like(z)
        with torch.no_grad():
            got, want = fn.frequency_layernorm(z), reference_layernorm(z)
            rec["max_normalised_difference"] = float((got - want).abs().max() / want.abs().max())
            del got, want
            r = race({"native": lambda: fn.frequency_layernorm(z), "reference_ops": lambda: reference_layernorm(z),
                      "copy_16B_per_element": lambda: dst.copy_(z)}, 20)
        rec.update(r)
        rec["bytes_needed"] = 16 * n
        rates(rec, r, rec["bytes_needed"])
        for mode in ("eager", "graph"):
            rec[f"reference_over_native_{mode}"] = round(r["reference_ops"][mode]["median_ms"] / r["native"][mode]["median_ms"], 2)
            rec[f"native_over_copy_{mode}"] = round(r["native"][mode]["median_ms"] / r["copy_16B_per_element"][mode]["median_ms"], 2)
    elif kind == "layer":
        B, N, D, H = dims
        layer = pkg.FrequencyTransformerLayer(D, H, device=dev)
        x = crandn(B, N, D)
        w = [layer.q_proj_freq, layer.k_proj_freq, layer.v_proj_freq, layer.o_proj_freq]

        def reference_layer():
            qh, kh, vh = ((x @ t).view(B, N, H, D // H).transpose(1, 2) for t in w[:3])
            a = reference_attention(qh, kh, vh)
            return a.transpose(1, 2).contiguous().view(B, N, D) @ w[3]

        def gemms_only():
            return [x @ t for t in w]
        with torch.no_grad():
            got, want = layer.forward(x), reference_layer()
            rec["max_normalised_difference"] = float((got - want).abs().max() / want.abs().max())
            del got, want
            r = race({"native": lambda: layer.forward(x), "reference_ops": reference_layer, "four_gemms": gemms_only}, 20)
        rec.update(r)
        for mode in ("eager", "graph"):
            rec[f"reference_over_native_{mode}"] = round(r["reference_ops"][mode]["median_ms"] / r["native"][mode]["median_ms"], 2)
            rec[f"gemm_share_of_native_{mode}"] = round(r["four_gemms"][mode]["median_ms"] / r["native"][mode]["median_ms"], 2)
    else:
        sys.exit(f"unknown case {case!r}")
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="attn:8x8x4096x64,attn:8x8x512x64,ln:64x4096x256,layer:8x1024x512x8")
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
