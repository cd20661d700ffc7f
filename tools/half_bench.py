#!/usr/bin/env python3
"""fwd+bwd of SpectralMixingLayer in fp32, bf16 and fp16, same process, interleaved.

bench.py's protocol per dtype: warm-up steps, then K steps {y = layer(x); y.backward(g); zero grads} captured in one
hipGraph, one replay timed with events.  The three dtypes' graphs are replayed in turn, `--rounds` times; the line of a
(config, dtype) is the median over the rounds.  Every configuration runs in `--procs` fresh processes.
Algorithmic bytes per step: x read twice (forward, backward's g) ... precisely: forward reads x and writes y, backward
reads g and writes grad_x -- 4 tensors of B N D elements -- plus the saved spectrum's write and read (B k D complex64).

    python tools/half_bench.py [--configs c2,c3,c5] [--steps 20] [--warmup 5] [--rounds 5] [--procs 3] [--json OUT]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"c2": (64, 4096, 256, 128), "c3": (8, 65536, 256, 128), "c5": (64, 4096, 512, 256)}
DTYPES = ["float32", "bfloat16", "float16"]


def child(cfgs, steps, warmup, rounds):
    sys.path.insert(0, ROOT)
    import torch
    import tensor_cuda_fft_amd as pkg
    dev = torch.device("cuda:0")
    out = []
    for name in cfgs:
        B, N, D, F = CONFIGS[name]
        units = {}
        for dn in DTYPES:
            dt = getattr(torch, dn)
            torch.manual_seed(0)
            layer = pkg.SpectralMixingLayer(D, num_filters=F).to(dev)
            x = torch.randn(B, N, D, device=dev).to(dt).requires_grad_(True)
            g = torch.randn(B, N, D, device=dev).to(dt)

            def step(layer=layer, x=x, g=g):
                y = layer(x)
                y.backward(g)
                for q in (x, *layer.parameters()):
                    q.grad = None
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(warmup):
                    step()
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(steps):
                    step()
            graph.replay()
            torch.cuda.synchronize()
            units[dn] = (graph, layer, x, g)
        times = {dn: [] for dn in DTYPES}
        for _ in range(rounds):
            for dn in DTYPES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                units[dn][0].replay()
                e1.record()
                torch.cuda.synchronize()
                times[dn].append(e0.elapsed_time(e1) / steps)
        k = min(F, N // 2)
        for dn in DTYPES:
            es = 4 if dn == "float32" else 2
            nbytes = 4 * B * N * D * es + 2 * B * k * D * 8
            ms = statistics.median(times[dn])
            out.append({"config": name, "shape": [B, N, D, F], "dtype": dn, "step_ms": ms,
                        "rounds_ms": times[dn], "alg_bytes": nbytes, "alg_TBps": nbytes / ms / 1e9})
        del units
        torch.cuda.empty_cache()
    print("HALF_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,c5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    cfgs = a.configs.split(",")
    if a.child:
        child(cfgs, a.steps, a.warmup, a.rounds)
        return 0
    runs = []
    for p in range(a.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--configs", a.configs,
                            "--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:])
            return r.returncode
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("HALF_BENCH ")][-1]
        runs.append(json.loads(line[len("HALF_BENCH "):]))
    summary = []
    for i, row in enumerate(runs[0]):
        per = [run[i]["step_ms"] for run in runs]
        summary.append({k: row[k] for k in ("config", "shape", "dtype", "alg_bytes")} |
                       {"step_ms_per_process": per, "step_ms_median": statistics.median(per)})
    for name in cfgs:
        f32 = [s for s in summary if s["config"] == name and s["dtype"] == "float32"][0]["step_ms_median"]
        for s in summary:
            if s["config"] == name:
                s["speedup_vs_fp32"] = f32 / s["step_ms_median"]
                s["alg_TBps"] = s["alg_bytes"] / s["step_ms_median"] / 1e9
    for s in summary:
        print(f"{s['config']:3s} {s['dtype']:9s} step {s['step_ms_median']:.4f} ms  (processes: "
              + ", ".join(f"{v:.4f}" for v in s["step_ms_per_process"])
              + f")  x{s['speedup_vs_fp32']:.2f} vs fp32  {s['alg_TBps']:.2f} TB/s algorithmic")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"protocol": vars(a), "summary": summary, "runs": runs}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
