#!/usr/bin/env python3
"""Timing of the native codecs (functional.polar_range / polar_quantize / polar_dequantize / log8_encode_complex /
log8_decode_complex, csrc/smx_quant.hip) beside the reference's own op sequence on the same GPU (the torch composition the
package runs for what the kernels do not take) and beside a device copy of the bytes each has to move; and of
FrequencyLinearLayer beside nn.Linear.  Launched by hand, not a pass/fail test:

    python tests/tools/quant_bench.py [--cases codec:16777216,codec:838860,linear:8x1024x512] [--out profiles/quant_bench.txt]

codec:<n> times the codecs on n complex64 coefficients (16777216 = a 4096 x 4096 spectrum; 838860 = the kept set of sst at
sparsity 0.05 of it).  linear:<B>x<N>x<D> times FrequencyLinearLayer(D, D) forward and forward + backward beside nn.Linear;
the reference's own frequency_linear would allocate B N D D complex64 there (17 GB at 8x1024x512), so it is timed at
(1, 64, D) and reported as a comparison point, not a ratio.
Every case runs in a child process of its own under its own time limit; the first that fails, faults or runs out of time
ends the run (nothing more is started on the GPU after it).  One JSON line per case.  "eager": HIP events around one call,
host cost included, the candidates alternating inside each round; "graph": ten calls captured in one hipGraph, the replay
timed, per call.  Bytes, counted from the shapes: quantize and the log8 encoder read 8 and write 2 per element, the decoders
the reverse, the range reads 8; each copy yardstick moves exactly the codec's bytes with Tensor.copy_ (half read, half
written)."""
import argparse
import json
import math
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


def race(fns, runs, graphs=True):
    """{name: {"eager": stats, "graph": stats}}: the candidates alternate inside each round"""
    for f in fns.values():
        f(); f()
    gs = {n: graphed(f) for n, f in fns.items()} if graphs else {}
    for g in gs.values():
        g.replay()
    eager, graph = {n: [] for n in fns}, {n: [] for n in gs}
    for _ in range(runs):
        for n, f in fns.items():
            eager[n].append(events_ms(f))
        for n, g in gs.items():
            graph[n].append(events_ms(g.replay) / GRAPH_CALLS)
    return {n: dict(eager=stats(eager[n]), **({"graph": stats(graph[n])} if graphs else {})) for n in fns}


def reference_range(z):
    import torch
    log_mag = torch.log2(torch.abs(z).clamp(min=1e-9))
    return log_mag.min(), log_mag.max()                       # (the reference reads each back with .item())


def reference_quantize(z, mag_bits, phase_bits, rng):
    import torch
    lm, lp = 2 ** mag_bits - 1, 2 ** phase_bits - 1
    mag, phase = torch.abs(z), torch.angle(z)
    log_mag = torch.log2(mag.clamp(min=1e-9))
    mag_norm = (log_mag - rng[0]) / (rng[1] - rng[0] + 1e-9)
    mag_q = (mag_norm * lm).round().clamp(0, lm).to(torch.uint8)
    phase_norm = (phase + math.pi) / (2 * math.pi)
    return mag_q, (phase_norm * lp).round().clamp(0, lp).to(torch.uint8)


def reference_dequantize(mag_q, phase_q, mag_bits, phase_bits, rng):
    import torch
    log_mag = mag_q.float() / (2 ** mag_bits - 1) * (rng[1] - rng[0]) + rng[0]
    return torch.polar(2.0 ** log_mag, phase_q.float() / (2 ** phase_bits - 1) * 2 * math.pi - math.pi)


def reference_log8_encode(x):
    import torch
    sign = (x >= 0).to(torch.uint8)
    quantized = ((torch.log2(torch.abs(x) + 1e-8) + 8) / 16 * 127).clamp(0, 127).to(torch.uint8)
    return (sign << 7) | quantized


def reference_log8_decode(e):
    import torch
    sign = ((e >> 7) & 1).to(torch.float32) * 2 - 1
    return sign * torch.pow(2.0, ((e & 0x7F).to(torch.float32) / 127) * 16 - 8)


def codec(n, rec):
    import torch
    from tensor_cuda_fft_amd import functional as fn
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1234)
    z = torch.complex(torch.randn(n, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen)) * 0.5
    bits = (4, 8)
    rng = tuple(fn.polar_range(z).tolist())
    mag_q, phase_q = fn.polar_quantize(z, *bits, rng)
    ref_q = reference_quantize(z, *bits, rng)
    rec["codes_that_differ_from_the_torch_ops"] = [int((a != b).sum()) for a, b in zip((mag_q, phase_q), ref_q)]
    re_q, im_q = fn.log8_encode_complex(z)
    src10, dst10 = (torch.empty(5 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    src8, dst8 = (torch.empty(4 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    r = race({
        "range": lambda: fn.polar_range(z), "range_reference_ops": lambda: reference_range(z),
        "copy_8_bytes": lambda: dst8.copy_(src8),
        "quantize": lambda: fn.polar_quantize(z, *bits, rng), "quantize_reference_ops": lambda: reference_quantize(z, *bits, rng),
        "dequantize": lambda: fn.polar_dequantize(mag_q, phase_q, *bits, rng),
        "dequantize_reference_ops": lambda: reference_dequantize(mag_q, phase_q, *bits, rng),
        "log8_encode": lambda: fn.log8_encode_complex(z),
        "log8_encode_reference_ops": lambda: (reference_log8_encode(z.real), reference_log8_encode(z.imag)),
        "log8_decode": lambda: fn.log8_decode_complex(re_q, im_q),
        "log8_decode_reference_ops": lambda: torch.complex(reference_log8_decode(re_q), reference_log8_decode(im_q)),
        "copy_10_bytes": lambda: dst10.copy_(src10)}, 20)
    rec.update(r)
    for name, nbytes, copy in (("range", 8 * n, "copy_8_bytes"), ("quantize", 10 * n, "copy_10_bytes"),
                               ("dequantize", 10 * n, "copy_10_bytes"), ("log8_encode", 10 * n, "copy_10_bytes"),
                               ("log8_decode", 10 * n, "copy_10_bytes")):
        for mode in ("eager", "graph"):
            t = r[name][mode]["median_ms"]
            rec[name][mode]["GBps"] = round(nbytes / t / 1e6, 1)
            rec[name][mode]["over_copy"] = round(t / r[copy][mode]["median_ms"], 2)
            rec[name][mode]["reference_ops_over_native"] = round(r[name + "_reference_ops"][mode]["median_ms"] / t, 2)


def linear(dims, rec):
    import torch
    import tensor_cuda_fft_amd as pkg
    B, N, D = dims
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    layer = pkg.FrequencyLinearLayer(D, D, sparsity=0.05).to(dev)
    dense = torch.nn.Linear(D, D).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(B, N, D, device=dev, generator=gen)
    xg = x.clone().requires_grad_()
    g = torch.randn(B, N, D, device=dev, generator=gen)

    def fwd_bwd(m):
        return lambda: torch.autograd.grad(m(xg), [xg] + list(m.parameters()), g)
    with torch.no_grad():
        rec.update(race({"layer_forward": lambda: layer(x), "nn_linear_forward": lambda: dense(x)}, 20))
    rec.update(race({"layer_forward_backward": fwd_bwd(layer), "nn_linear_forward_backward": fwd_bwd(dense)}, 20, graphs=False))
    xs = x[:1, :64].contiguous()

    def reference(xr, w_freq, bias):                          # fft_tensor/zero_materialize.py:66-84, the broadcast product
        y_freq = (torch.fft.fft(xr, dim=-1).unsqueeze(-1) * w_freq.unsqueeze(0).unsqueeze(0)).sum(dim=2)
        return torch.fft.ifft(y_freq, dim=-1).real + bias
    with torch.no_grad():
        rec["comparison_point_1x64"] = race({"reference_ops_torch_fft": lambda: reference(xs, layer.weight_freq, layer.bias),
                                             "layer_forward": lambda: layer(xs)}, 10)
        d = (layer(xs) - reference(xs, layer.weight_freq, layer.bias)).abs().max() / reference(xs, layer.weight_freq, layer.bias).abs().max()
    rec["comparison_point_1x64"]["max_normalised_difference"] = float(d)
    rec["reference_intermediate_bytes_at_full_shape"] = 8 * B * N * D * D
    rec["layer_over_nn_linear_forward"] = round(rec["layer_forward"]["graph"]["median_ms"]
                                                / rec["nn_linear_forward"]["graph"]["median_ms"], 2)


def step(case):
    sys.path.insert(0, ROOT)
    kind, _, dims = case.partition(":")
    rec = {"step": case}
    if kind == "codec":
        codec(int(dims), rec)
    elif kind == "linear":
        linear(tuple(int(v) for v in dims.split("x")), rec)
    else:
        sys.exit(f"unknown case {case!r}")
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="codec:16777216,codec:838860,linear:8x1024x512")
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
