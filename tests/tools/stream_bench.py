#!/usr/bin/env python3
"""Timing of the backbone update per emitted chunk (tensor_cuda_fft_amd.streaming.update_backbone_chunk) at fft_lm's
generation shape -- seq_len 1024, kernel_len 128, d_model 512, 6 layers, chunk 16 -- for Bt = 1 and 8, three ways:

    native_eager   the two native launches per layer around torch's GEMV / linears, launched from Python
    native_graph   the same update replayed from one captured graph (no host share)
    torch_fft      the reference's op sequence (scripts/generate_chunked_overlap_save.py:78-206: LayerNorm, torch.cat of
                   the window, the full sum, rfft / irfft of n_fft points, the pointwise chain, with its k_freq / g_freq /
                   gain caches) restated with torch.fft on the same GPU -- a comparison point only, never part of the
                   product

Device events around --reps back-to-back updates (a sizeable fraction of a second), after a warm-up; the three variants
alternate over --rounds rounds in one process and the median round is reported, per chunk.  Launched by hand:

    python tests/tools/stream_bench.py [--reps 200] [--rounds 5] [--batches 1,8]

--kernels-only runs 50 native updates and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse, json, os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import tensor_cuda_fft_amd as pkg


def torch_fft_update(backbone, st, ids, caches):
    """st: per layer {"ctx_ln" (Bt, T, C), "ctx_sum"}; returns h_last"""
    h = backbone.embed(ids)
    n = ids.shape[1]
    K = backbone.cfg.kernel_len
    for blk, s, c in zip(backbone.blocks, st, caches):
        ln_chunk = blk.ln(h)
        ctx = torch.cat([s["ctx_ln"][:, n:], ln_chunk], dim=1)
        ctx_sum = ctx.sum(dim=1)
        g_ctx = torch.sigmoid(blk.gate_ctx(ctx_sum / float(ctx.shape[1])))
        seg = torch.cat([ctx[:, -(K - 1 + n):-n], ln_chunk], dim=1)
        x_freq = torch.fft.rfft(F.pad(seg, (0, 0, 0, c["n_fft"] - seg.shape[1])), dim=1)
        y_freq = x_freq * c["k_freq"].view(1, -1, 1) * c["gain"].view(1, 1, -1)
        y_freq = y_freq * c["g_freq"].view(1, -1, 1) * g_ctx.unsqueeze(1)
        y = torch.fft.irfft(y_freq, n=c["n_fft"], dim=1)[:, K - 1:K - 1 + n]
        h_out = h + y
        h = h_out + blk.ffn(blk.ffn_ln(h_out))
        s["ctx_ln"], s["ctx_sum"] = ctx.contiguous(), ctx_sum.contiguous()
    return backbone.ln_f(h)[:, -1].contiguous()


def timed(step, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = pkg.LMConfig()
    chunk = 16
    backbone = pkg.FixedSpectralLM(cfg).to(dev).eval()
    with torch.no_grad():
        for blk in backbone.blocks:
            blk.kernel.normal_(0.0, 0.3)
            blk.gate_freq_logits.normal_(0.5, 1.0)
            blk.gate_ctx.weight.normal_(0.0, 0.02)
    n_fft = pkg.fixed_spectral.next_pow2(cfg.seq_len + cfg.kernel_len - 1)
    for Bt in map(int, args.batches.split(",")):
        ids0 = torch.randint(0, 256, (Bt, cfg.seq_len), device=dev)
        ids = torch.randint(0, 256, (Bt, chunk), device=dev)
        with torch.no_grad():
            states = pkg.init_layer_states(backbone, ids0, chunk)
            assert states.native
            native = lambda: pkg.update_backbone_chunk(backbone, states, ids)
            if args.kernels_only:
                for _ in range(50):
                    native()
                torch.cuda.synchronize()
                continue
            gstates = states.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    pkg.update_backbone_chunk(backbone, gstates, ids)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                pkg.update_backbone_chunk(backbone, gstates, ids)
            ref_st, caches, h = [], [], backbone.embed(ids0)
            for blk in backbone.blocks:
                ln_in = blk.ln(h)
                ref_st.append({"ctx_ln": ln_in.contiguous(), "ctx_sum": ln_in.sum(dim=1)})
                k = torch.zeros(n_fft, device=dev)
                k[:cfg.kernel_len] = blk.kernel
                caches.append({"n_fft": n_fft, "k_freq": torch.fft.rfft(k), "gain": blk.gain.detach(),
                               "g_freq": torch.sigmoid(blk.gate_freq_logits[:n_fft // 2 + 1])})
                h = blk(h)
            variants = {"native_eager": native, "native_graph": graph.replay,
                        "torch_fft": lambda: torch_fft_update(backbone, ref_st, ids, caches)}
            for f in variants.values():                                   # warm-up
                for _ in range(10):
                    f()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, f in variants.items():
                    ms[k].append(timed(f, args.reps))
        rec = {"op": "backbone update per chunk", "Bt": Bt, "seq_len": cfg.seq_len, "kernel_len": cfg.kernel_len,
               "d_model": cfg.d_model, "layers": cfg.n_layers, "chunk": chunk, "reps": args.reps, "rounds": args.rounds}
        for k, v in ms.items():
            v = sorted(v)
            rec[k + "_ms"] = round(v[len(v) // 2], 4)
            rec[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        rec["torch_fft_over_native_graph"] = round(rec["torch_fft_ms"] / rec["native_graph_ms"], 2)
        rec["torch_fft_over_native_eager"] = round(rec["torch_fft_ms"] / rec["native_eager_ms"], 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
