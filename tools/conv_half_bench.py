#!/usr/bin/env python3
"""fwd+bwd of causal_spectral_conv (FixedSpectralBlock's convolution) with fp32, bf16 and fp16 activations, same process,
interleaved.

Five variants per shape: fp32; bf16 and fp16 on the native 2-byte rows (k_conv1's IO instances); bf16 and fp16 on the
up-cast route (x.float() -> the fp32 op -> .to(dtype), what a caller without the 2-byte kernels would write).  The
parameters (taps, gain, gate logits) and the context gate stay fp32 in every variant.  tools/half_bench.py's protocol:
warm-up steps, then K steps {y = conv(x, ...); y.backward(g); drop grads} captured in one hipGraph, one replay timed
with events; the variants' graphs are replayed in turn, `--rounds` times; the line of a (shape, variant) is the median
over the rounds, and every shape runs in `--procs` fresh processes.
Algorithmic bytes per step of the convolution launches: forward reads x and writes y, backward reads g and writes
grad_x (4 tensors of B T C elements), plus the saved packed spectrum written once and read once.

    python tools/conv_half_bench.py [--configs f2,fb,fold,n1k] [--steps 20] [--warmup 5] [--rounds 5] [--procs 3]
                                    [--json OUT]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"f2": (64, 1024, 512, 128),       # bench.py's f2 row, n_fft 2048
           "fb": (8, 1024, 512, 128),        # fft_lm's default batch
           "fold": (32, 1920, 512, 128),     # rows > n_fft / 2: folded
           "n1k": (64, 768, 256, 128)}       # n_fft 1024
VARIANTS = ["fp32", "bf16", "fp16", "bf16_upcast", "fp16_upcast"]


def child(cfgs, steps, warmup, rounds):
    sys.path.insert(0, ROOT)
    import torch
    from tensor_cuda_fft_amd import _lib, functional
    from tensor_cuda_fft_amd.fixed_spectral import causal_spectral_conv, next_pow2
    dev = torch.device("cuda:0")
    out = []
    for name in cfgs:
        B, T, C, K = CONFIGS[name]
        n = next_pow2(T + K - 1)
        fb = n // 2 + 1
        _, saveb = functional._conv_plan(B, T, C, n)
        units = {}
        for vn in VARIANTS:
            dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[vn.split("_")[0]]
            up = vn.endswith("_upcast")
            torch.manual_seed(0)
            x = torch.randn(B, T, C, device=dev).to(dt).requires_grad_(True)
            g = torch.randn(B, T, C, device=dev).to(dt)
            kernel = (torch.randn(K, device=dev) * 0.05).requires_grad_(True)
            gain = torch.ones(C, device=dev, requires_grad=True)
            logits = torch.full((fb,), 2.0, device=dev, requires_grad=True)
            g_ctx = torch.rand(B, C, device=dev, requires_grad=True)
            leaves = (x, kernel, gain, logits, g_ctx)

            def step(x=x, g=g, kernel=kernel, gain=gain, logits=logits, g_ctx=g_ctx, up=up, dt=dt, leaves=leaves):
                if up:
                    y = causal_spectral_conv(x.float(), kernel, gain, logits, g_ctx).to(dt)
                else:
                    y = causal_spectral_conv(x, kernel, gain, logits, g_ctx)
                y.backward(g)
                for q in leaves:
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
            units[vn] = (graph, leaves, g)
        times = {vn: [] for vn in VARIANTS}
        for _ in range(rounds):
            for vn in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                units[vn][0].replay()
                e1.record()
                torch.cuda.synchronize()
                times[vn].append(e0.elapsed_time(e1) / steps)
        native = {io: _lib.conv_io_supported(B, T, C, n, io) for io in (1, 2)}
        for vn in VARIANTS:
            es = 4 if vn == "fp32" else 2
            nbytes = 4 * B * T * C * es + 2 * saveb
            ms = statistics.median(times[vn])
            out.append({"config": name, "shape": [B, T, C, K], "n_fft": n, "variant": vn, "step_ms": ms,
                        "rounds_ms": times[vn], "alg_bytes": nbytes, "native_io": native,
                        "alg_TBps": nbytes / ms / 1e9})
        del units
        torch.cuda.empty_cache()
    print("CONV_HALF_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="f2,fb,fold,n1k")
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
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CONV_HALF_BENCH ")][-1]
        runs.append(json.loads(line[len("CONV_HALF_BENCH "):]))
    summary = []
    for i, row in enumerate(runs[0]):
        per = [run[i]["step_ms"] for run in runs]
        summary.append({k: row[k] for k in ("config", "shape", "n_fft", "variant", "alg_bytes", "native_io")} |
                       {"step_ms_per_process": per, "step_ms_median": statistics.median(per)})
    for name in cfgs:
        rows = {s["variant"]: s for s in summary if s["config"] == name}
        for s in rows.values():
            s["speedup_vs_fp32"] = rows["fp32"]["step_ms_median"] / s["step_ms_median"]
            s["alg_TBps"] = s["alg_bytes"] / s["step_ms_median"] / 1e9
            if not s["variant"].endswith("_upcast") and s["variant"] != "fp32":
                s["speedup_vs_upcast"] = rows[s["variant"] + "_upcast"]["step_ms_median"] / s["step_ms_median"]
    for s in summary:
        print(f"{s['config']:4s} {str(tuple(s['shape'])):20s} {s['variant']:11s} step {s['step_ms_median']:.4f} ms "
              f"(processes: " + ", ".join(f"{v:.4f}" for v in s["step_ms_per_process"])
              + f")  x{s['speedup_vs_fp32']:.2f} vs fp32"
              + (f"  x{s['speedup_vs_upcast']:.2f} vs up-cast" if "speedup_vs_upcast" in s else "")
              + f"  {s['alg_TBps']:.2f} TB/s algorithmic")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"protocol": vars(a), "summary": summary, "runs": runs}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
