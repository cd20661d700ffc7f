#!/usr/bin/env python3
"""Timing of the native row transform (functional.row_fft_raw, csrc/smx_rowfft.hip) beside the path the same rows took
before it -- the sequence transform on a one-channel batch, seq_fft_raw(z.unsqueeze(-1)), which stays reachable --, beside
a device copy of the bytes the transform has to move (the floor the package's streaming ops are quoted against) and beside
torch.fft.fft(dim=-1) as a comparison point.  Launched by hand, not a pass/fail test:

    python tests/tools/rowfft_bench.py [--cases 4096x4096,65536x256,1048576x16,4096x4096:c2r,4096x4096:r2c] [--out profiles/rowfft_bench.txt]

<rows>x<n> is the complex transform; :c2r adds conj_in + real_out + scale (frequency_ops.ifft_last_real: 8 bytes read, 4
written per point) against today's composition with its conjugation, real part and division; :r2c reads fp32 rows (4 read,
8 written) against the complex copy followed by the sequence transform.  A sweep, `--cases sweep`, times 2^24 points at every
supported length: the table the callers' dispatch is read from (recorded as profiles/rowfft_sweep.txt; `--cases
default,sweep` runs both lists into one file).
Every case runs in a child process of its own under its own time limit; the first that fails, faults or runs out of time
ends the run (nothing more is started on the GPU after it).  One JSON line per case.  "eager": HIP events around one call,
host cost included, the candidates alternating inside each round; "graph": ten calls captured in one hipGraph, the replay
timed, per call.  The copy yardstick moves exactly the transform's bytes with Tensor.copy_ (half read, half written)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMIT = 300                                                   # seconds per child
GRAPH_CALLS = 10
DEFAULT = "4096x4096,65536x256,1048576x16,4096x4096:c2r,4096x4096:r2c"
SWEEP = ",".join(f"{(1 << 24) >> i}x{1 << i}" for i in range(1, 13))


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
    gs = {n: graphed(f) for n, f in fns.items()}
    for g in gs.values():
        g.replay()
    eager, graph = {n: [] for n in fns}, {n: [] for n in gs}
    for _ in range(runs):
        for n, f in fns.items():
            eager[n].append(events_ms(f))
        for n, g in gs.items():
            graph[n].append(events_ms(g.replay) / GRAPH_CALLS)
    return {n: {"eager": stats(eager[n]), "graph": stats(graph[n])} for n in fns}


def step(case):
    sys.path.insert(0, ROOT)
    import torch
    from tensor_cuda_fft_amd import functional as fn
    shape, _, kind = case.partition(":")
    rows, n = (int(v) for v in shape.split("x"))
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(rows, n, device=dev, generator=gen)
    z = torch.complex(x, torch.randn(rows, n, device=dev, generator=gen))
    if kind == "c2r":
        native = lambda: fn.row_fft_raw(z, conj_in=True, real_out=True, scale=1.0 / n)
        before = lambda: fn.seq_fft_raw(z.conj().resolve_conj().unsqueeze(-1)).squeeze(-1).real / n
        torch_fft = lambda: torch.fft.ifft(z, dim=-1).real
        nbytes = 12 * rows * n
    elif kind == "r2c":
        native = lambda: fn.row_fft_raw(x)
        before = lambda: fn.seq_fft_raw(x.to(torch.complex64).unsqueeze(-1)).squeeze(-1)
        torch_fft = lambda: torch.fft.fft(x, dim=-1)
        nbytes = 12 * rows * n
    elif kind == "":
        native = lambda: fn.row_fft_raw(z)
        before = lambda: fn.seq_fft_raw(z.unsqueeze(-1)).squeeze(-1)
        torch_fft = lambda: torch.fft.fft(z, dim=-1)
        nbytes = 16 * rows * n
    else:
        sys.exit(f"unknown case {case!r}")
    src, dst = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    a, b = native(), before()
    rec = {"step": case, "max_normalised_difference_native_to_the_path_before": float((a - b).abs().max() / b.abs().max())}
    r = race({"row_fft_raw": native, "seq_fft_raw_one_channel": before, "copy_of_the_bytes": lambda: dst.copy_(src),
              "torch_fft": torch_fft}, 20)
    rec.update(r)
    for mode in ("eager", "graph"):
        t = r["row_fft_raw"][mode]["median_ms"]
        rec["row_fft_raw"][mode]["GBps"] = round(nbytes / t / 1e6, 1)
        rec["row_fft_raw"][mode]["over_copy"] = round(t / r["copy_of_the_bytes"][mode]["median_ms"], 2)
        rec["row_fft_raw"][mode]["path_before_over_native"] = round(r["seq_fft_raw_one_channel"][mode]["median_ms"] / t, 2)
        rec["row_fft_raw"][mode]["torch_fft_over_native"] = round(r["torch_fft"][mode]["median_ms"] / t, 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT, help="comma-separated <rows>x<n>[:c2r|:r2c]; `default` and `sweep` name the two lists")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return step(args.child)
    lines = []
    named = {"default": DEFAULT, "sweep": SWEEP}
    for case in filter(None, ",".join(named.get(c, c) for c in args.cases.split(",")).split(",")):
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
