#!/usr/bin/env python3
"""Timing of the epoch-end pieces (training.parroting_score's search and training.eval_loss).  Launched by hand:

    python tests/tools/eval_bench.py [--sizes 16,256,1024] [--out profiles/eval_bench.txt]

Every GPU step runs in a child process of its own under its own time limit; the first step that fails, faults or runs
out of time ends the run (nothing more is started on the GPU after it).  One JSON line per step.

search:<MiB>  functional.find_snippets (smx_match_first) over a corpus of that size built ON THE DEVICE from a seeded byte
    distribution (64 table entries: lower-case letters by rough English frequency, blanks, a line feed), for S = 23 (what
    the default generation gives: 416-464 bytes hold 23 candidates) and S = 64 snippets of 64 bytes.  The snippets are
    drawn from the same distribution -- so their first words do occur in the corpus and candidates are verified, as with
    text -- and carry one byte the table lacks: every snippet is absent, the case that costs the reference a full scan
    each.  HIP events around each call, the search and the two yardsticks alternating; median, minimum and count are printed.
    (a) `bytes.find` per snippet on the host copy: the reference's operation (fft_lm/train_fixed_full.py:200-204), wall
        clock.
    (b) `corpus.clone()` on the same device: a plain pass that moves 2 bytes per corpus byte -- a yardstick only.
    (c) `corpus.view(torch.int64).sum()`: torch's reduction over the same bytes, a pass that only reads -- the second
        yardstick, what "a plain read" means in DESIGN.md section 7m.
eval_loss  training.eval_loss of a FixedSpectralLM(TrainConfig()) (6 layers, d_model 512, windows of 1024, batch 8) at
    val_batches = 20 over a 16 MiB corpus on the device, against the same loop reading each batch's loss with .item() as
    the reference does (:181); host clock around calls that end in a synchronise, alternating.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TABLE = b"eeeeeeetttttaaaaooooiiiinnnnsssshhhrrrddlluucmwfgypbvk" + b" " * 9 + b"\n"
MISSING = ord("#")
LIMITS = {"search": 420, "eval_loss": 420}                  # seconds per child


def device_corpus(n, seed, dev):
    import torch
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    table = torch.tensor(list(TABLE), dtype=torch.uint8, device=dev)
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    step = 32 << 20
    for i in range(0, n, step):
        m = min(step, n - i)
        out[i:i + m] = table[torch.randint(0, len(TABLE), (m,), device=dev, generator=gen)]
    return out


def events_ms(f):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "runs": len(ts)}


def step_search(mib):
    import torch
    sys.path.insert(0, ROOT)
    import tensor_cuda_fft_amd as pkg
    dev = torch.device("cuda:0")
    n = mib << 20
    corpus = device_corpus(n, 1234, dev)
    runs = 20 if mib <= 16 else 10 if mib <= 256 else 5
    rec = {"step": f"search:{mib}", "corpus_MiB": mib, "L": 64}
    blob = bytes(corpus.cpu().numpy().tobytes())
    for S in (23, 64):
        snips = device_corpus(S * 64, 99 + S, dev).view(S, 64).clone()
        snips[:, 10] = MISSING
        host_snips = [bytes(r.tolist()) for r in snips.cpu()]
        for _ in range(2):
            first = pkg.find_snippets(corpus, snips)
            corpus.clone()
        torch.cuda.synchronize()
        words = corpus.view(torch.int64)
        words.sum()
        search, clone, read = [], [], []
        for _ in range(runs):
            search.append(events_ms(lambda: pkg.find_snippets(corpus, snips)))
            clone.append(events_ms(lambda: corpus.clone()))
            read.append(events_ms(lambda: words.sum()))
        host_runs = 3 if mib <= 16 else 1
        host = []
        for _ in range(host_runs):
            t0 = time.perf_counter()
            found = [blob.find(s) for s in host_snips]
            host.append((time.perf_counter() - t0) * 1e3)
        assert first.cpu().tolist() == found == [-1] * S
        s, c, r, h = stats(search), stats(clone), stats(read), stats(host)
        rec[f"S{S}"] = {"find_snippets": s, "clone": c, "read_sum": r, "host_find_loop": h,
                        "search_GBps": round(n / s["median_ms"] / 1e6, 1),
                        "clone_read_GBps": round(n / c["median_ms"] / 1e6, 1),
                        "read_sum_GBps": round(n / r["median_ms"] / 1e6, 1),
                        "search_over_clone": round(s["median_ms"] / c["median_ms"], 2),
                        "search_over_read_sum": round(s["median_ms"] / r["median_ms"], 2),
                        "host_over_search": round(h["median_ms"] / s["median_ms"], 1)}
    print(json.dumps(rec), flush=True)


def step_eval_loss():
    import torch
    sys.path.insert(0, ROOT)
    import tensor_cuda_fft_amd as pkg
    dev = torch.device("cuda:0")
    cfg = pkg.TrainConfig(device="cuda")
    torch.manual_seed(cfg.seed)
    model = pkg.FixedSpectralLM(cfg).to(dev)
    corpus = device_corpus(16 << 20, 4321, dev)
    starts = pkg.make_val_starts(corpus.numel(), cfg.seq_len, cfg.val_windows, cfg.seed + 1)

    @torch.no_grad()
    def per_batch_item():
        """the same loop with the reference's host read per batch"""
        model.eval()
        sel = starts[torch.randperm(starts.numel())[: cfg.val_batches * cfg.batch_size]]
        losses = []
        for i in range(0, sel.numel(), cfg.batch_size):
            x, y = pkg.sample_windows(corpus, sel[i:i + cfg.batch_size], cfg.seq_len)
            losses.append(float(pkg.cross_entropy(model(x, cutoff=None), y).item()))
        return sum(losses) / max(1, len(losses))

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    ours = lambda: pkg.eval_loss(model, corpus, starts, cfg, None)
    torch.manual_seed(1); a = ours()
    torch.manual_seed(1); b = per_batch_item()
    assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    t_ours, t_item = [], []
    for _ in range(5):
        t_ours.append(wall(ours)[0])
        t_item.append(wall(per_batch_item)[0])
    print(json.dumps({"step": "eval_loss", "model": "FixedSpectralLM(TrainConfig())", "batch": [cfg.batch_size, cfg.seq_len],
                      "val_batches": cfg.val_batches, "loss": round(a, 6), "eval_loss": stats(t_ours),
                      "loop_with_item_per_batch": stats(t_item)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,256,1024", help="corpus sizes in MiB")
    ap.add_argument("--no-eval-loss", action="store_true")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, _, arg = args.child.partition(":")
        return step_search(int(arg)) if kind == "search" else step_eval_loss()
    steps = [f"search:{int(s)}" for s in args.sizes.split(",") if s] + ([] if args.no_eval_loss else ["eval_loss"])
    lines = []
    for step in steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], capture_output=True,
                               text=True, timeout=LIMITS[step.partition(":")[0]])
        except subprocess.TimeoutExpired:
            sys.exit(f"{step}: no result within its time limit; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"{step}: exit status {r.returncode}; nothing more is started\n{r.stderr[-3000:]}")
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        print("\n".join(out), flush=True)
        lines += out
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
