#!/usr/bin/env python3
"""Timing of the sparse spectral tensor's native steps (csrc/smx_sst.hip) beside the reference's torch sequences on the
same spectrum and the same GPU.  Launched by hand, not a pass/fail test:

    python tests/tools/sst_bench.py [--cases 1024x1024:0.05,4096x4096:0.01,4096x4096:0.05] [--out profiles/sst_bench.txt]

Every case runs in a child process of its own under its own time limit; the first that fails, faults or runs out of
time ends the run (nothing more is started on the GPU after it).  One JSON line per case.  HIP events around each call
(host clock around calls that end in a host read), the native step and its yardsticks alternating; median, minimum and
count are printed.  Bytes are counted from the shapes: n = H W elements of 8 bytes.

sparsify     functional.sparsify_topk (three select passes, a count pass and a write pass over the spectrum: 5 x 8 n bytes
             read, 16 m written; one host read of m) beside
             (a) the reference's five ops (fft_tensor/tensor.py:138-144: abs, topk(k).values[-1], >=, nonzero, freq[mask]),
             (b) spectrum.view(int64).sum(): a pass that only reads the 8 n bytes -- the floor of ONE pass.
scatter      functional.sparse_scatter(assume_ascending=True) (8 n bytes written once, 16 m read) beside
             (a) zeros + index_put_ (the reference's _scatter_pytorch), (b) out.zero_(): the floor.
sst / to_spatial   sst(x) and t.to_spatial() whole (host clock), and their parts: functional.fftn, sparsify_topk;
             sparse_scatter, functional.ifftn -- the transform is the axis-by-axis composition of the sequence
             transform, whose speed is not the subject of smx_sst.hip.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMIT = 420                                                   # seconds per child


def events_ms(f):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "runs": len(ts)}


def reference_sparsify(freq, k):
    """the reference's five ops (fft_tensor/tensor.py:138-144)"""
    import torch
    magnitude = torch.abs(freq)
    threshold = torch.topk(magnitude.flatten(), k).values[-1]
    mask = magnitude >= threshold
    return freq[mask], torch.nonzero(mask, as_tuple=False)


def step(case):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tensor_cuda_fft_amd as pkg
    import sst_common as sc
    dims, _, sp = case.partition(":")
    H, W = (int(v) for v in dims.split("x"))
    sparsity = float(sp)
    dev = torch.device("cuda:0")
    n = H * W
    k = max(1, int(n * sparsity))
    runs = 20 if n <= 1 << 20 else 8
    x = torch.randn(H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    freq = pkg.fftn(x.to(torch.complex64))
    words = freq.view(-1).view(torch.int64)
    rec = {"step": case, "n": n, "k": k, "bytes_per_pass": 8 * n}

    # sparsify
    for _ in range(2):
        c, i = pkg.sparsify_topk(freq, sparsity)
        rc, ri = reference_sparsify(freq, k)
        words.sum()
    m = int(i.numel())
    # same membership up to the tie rule (squared key against torch.abs): entries may differ only within BAND of the
    # reference threshold (a spectrum of this size holds many more than BAND_CAP entries there: the cap is not applied)
    import numpy as np
    magnitude = torch.abs(freq).cpu().numpy().reshape(-1)
    ref_flat = (ri[:, 0] * W + ri[:, 1]).cpu().numpy()
    thr = float(magnitude[ref_flat].min())
    differ = np.setxor1d(i.cpu().numpy(), ref_flat)
    assert (np.abs(magnitude[differ].astype(np.float64) - thr) <= sc.BAND * thr).all()
    rec["membership_differs_from_reference"] = int(differ.size)
    ours, ref, read = [], [], []
    for _ in range(runs):
        ours.append(wall_ms(lambda: pkg.sparsify_topk(freq, sparsity)))
        ref.append(wall_ms(lambda: reference_sparsify(freq, k)))
        read.append(events_ms(lambda: words.sum()))
    o, r, f = stats(ours), stats(ref), stats(read)
    rec["sparsify"] = {"m": m, "sparsify_topk": o, "reference_five_ops": r, "read_sum": f,
                       "bytes_moved": 5 * 8 * n + 16 * m,
                       "sparsify_GBps": round((5 * 8 * n + 16 * m) / o["median_ms"] / 1e6, 1),
                       "read_sum_GBps": round(8 * n / f["median_ms"] / 1e6, 1),
                       "sparsify_over_read_sum": round(o["median_ms"] / f["median_ms"], 2),
                       "reference_over_sparsify": round(r["median_ms"] / o["median_ms"], 2)}

    # scatter
    def torch_scatter():
        out = torch.zeros(n, dtype=torch.complex64, device=dev)
        out.index_put_((i,), c)
        return out
    buf = torch.empty(n, dtype=torch.complex64, device=dev)
    for _ in range(2):
        got = pkg.sparse_scatter(c, i, (H, W), assume_ascending=True)
        want = torch_scatter()
        buf.zero_()
    assert torch.equal(got.view(-1), want)
    ours, ref, fill = [], [], []
    for _ in range(runs):
        ours.append(events_ms(lambda: pkg.sparse_scatter(c, i, (H, W), assume_ascending=True)))
        ref.append(events_ms(torch_scatter))
        fill.append(events_ms(lambda: buf.zero_()))
    o, r, f = stats(ours), stats(ref), stats(fill)
    rec["scatter"] = {"sparse_scatter": o, "zeros_index_put": r, "zero_fill": f, "bytes_moved": 8 * n + 16 * m,
                      "scatter_GBps": round((8 * n + 16 * m) / o["median_ms"] / 1e6, 1),
                      "zero_fill_GBps": round(8 * n / f["median_ms"] / 1e6, 1),
                      "scatter_over_zero_fill": round(o["median_ms"] / f["median_ms"], 2),
                      "reference_over_scatter": round(r["median_ms"] / o["median_ms"], 2)}

    # the tensor whole, and its parts
    z = x.to(torch.complex64)
    t = pkg.sst(x, sparsity=sparsity)
    t.to_spatial()
    whole_sst, whole_sp, fwd, inv = [], [], [], []
    for _ in range(max(3, runs // 4)):
        whole_sst.append(wall_ms(lambda: pkg.sst(x, sparsity=sparsity)))
        whole_sp.append(wall_ms(t.to_spatial))
        fwd.append(events_ms(lambda: pkg.fftn(z)))
        inv.append(events_ms(lambda: pkg.ifftn(got)))
        pkg.MemoryManager.clear_all()
    rec["tensor"] = {"sst": stats(whole_sst), "to_spatial": stats(whole_sp), "fftn": stats(fwd), "ifftn": stats(inv),
                     "sparsify_topk": rec["sparsify"]["sparsify_topk"], "sparse_scatter": rec["scatter"]["sparse_scatter"]}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x1024:0.05,4096x4096:0.01,4096x4096:0.05", help="HxW:sparsity, comma separated")
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
