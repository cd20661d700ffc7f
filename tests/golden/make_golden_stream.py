#!/usr/bin/env python3
"""Golden vectors of FixedSpectralLM and of the overlap-save chunk update, produced by the REFERENCE on CPU:
fft_lm/train_fixed_full.py:566-618 (FixedSpectralLM) and scripts/generate_chunked_overlap_save.py (init_layer_states
:51-74, overlap_save_block_update :78-176, update_backbone_chunk :179-206), eval mode, every parameter randomised
(tests/stream_common.py randomize).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stream.py [name prefixes]

The reference asserts one batch row: its states are built per row and stacked.  X05 runs under a cutoff: the blocks'
forward gets it at init, the update gets it folded into the reference's cache["g_freq"].
Beside the reference's fp32 results every fixture records `ref_err_<output>`: the max-normalised error of that fp32
result against an fp64 evaluation of the same op sequence (tests/stream_common.py, checked here to land on the
reference's own numbers in fp32).  The generator FAILS if one of them exceeds a quarter of the tolerance the tests
apply: the yardstick is never outside its own bound.  Arrays over 128 KiB go beside the .npz as <name>.<key>.npy
(conftest.load_golden), so that no committed file passes 1 MiB.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                     # noqa: E402  (puts the reference on sys.path)
from make_golden import SEED                                 # noqa: E402
import stream_common as sc                                   # noqa: E402
from conftest import TOL_ACT, rel_err                        # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    from fft_lm import train_fixed_full as tff               # noqa: E402
    import scripts.generate_chunked_overlap_save as gos      # noqa: E402
    from scripts.generate_chunked_overlap_save import init_layer_states, update_backbone_chunk   # noqa: E402

BESIDE = 128 * 1024


def save(name, rec):
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in rec.items()}
    for k in [k for k, a in arrs.items() if a.nbytes > BESIDE]:
        np.save(os.path.join(mg.OUT, f"{name}.{k}.npy"), arrs.pop(k))
    path = os.path.join(mg.OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def stream_case(name, Bt, T, K, C, chunk, layers, chunks, cutoff=None, trans=32):
    gen = torch.Generator().manual_seed(SEED)
    cfg = tff.TrainConfig(seq_len=T, kernel_len=K, d_model=C, n_layers=layers, jpeg_transition=trans)
    with contextlib.redirect_stdout(io.StringIO()):          # the constructor prints the architecture
        model = tff.FixedSpectralLM(cfg).eval()
    sc.randomize(model, gen)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ids = torch.randint(0, 256, (Bt, T), generator=gen)
    new_ids = torch.randint(0, 256, (chunks, Bt, chunk), generator=gen)
    n_fft = tff.conv_freq_bins(T, K) * 2 - 2
    L = K - 1 + chunk

    with torch.no_grad():
        rec = {"logits": model(ids, cutoff=cutoff), "hidden": model.forward_hidden(ids, cutoff=cutoff)}
        if cutoff is not None:                               # init_layer_states calls blk(h, cutoff=None)
            for blk in model.blocks:
                blk.forward = (lambda h, cutoff=None, _f=blk.forward, _c=cutoff: _f(h, cutoff=_c))
        rows = [init_layer_states(model, ids[b:b + 1]) for b in range(Bt)]
        if cutoff is not None:
            for st in rows:
                st["caches"] = [{"g_freq": torch.sigmoid(blk.gate_freq_logits[:n_fft // 2 + 1])
                                 * sc.mask_ref(cutoff, n_fft // 2 + 1, blk.transition_bins)} for blk in model.blocks]
        rec["h_last0"] = torch.cat([st["h_last"] for st in rows])
        h_out = torch.zeros(chunks, layers, Bt, chunk, C)
        h_last = torch.zeros(chunks, Bt, C)
        for c in range(chunks):
            for b in range(Bt):
                # each layer's output: the reference's own block update, traced through its caller
                trace = []
                orig = gos.overlap_save_block_update

                def traced(*a, _o=orig, **kw):
                    out = _o(*a, **kw)
                    trace.append(out[0])
                    return out
                gos.overlap_save_block_update = traced
                try:
                    rows[b] = update_backbone_chunk(model, rows[b], new_ids[c, b].tolist())
                finally:
                    gos.overlap_save_block_update = orig
                for li in range(layers):
                    h_out[c, li, b] = trace[li][0]
                h_last[c, b] = rows[b]["h_last"][0]
        rec.update({"h_out": h_out, "h_last": h_last,
                    "win_tail": torch.stack([torch.cat([st["layers"][li]["ctx_ln"][:, T - L:] for st in rows])
                                             for li in range(layers)]),
                    "ctx_sum": torch.stack([torch.cat([st["layers"][li]["ctx_sum"] for st in rows])
                                            for li in range(layers)])})

        def restate(dtype):
            out = {"hidden": sc.hidden_ref(sd, ids, layers, trans, cutoff, dtype)}
            out["logits"] = out["hidden"] @ sd["embed.weight"].to(dtype).T
            st = sc.init_ref(sd, ids, layers, trans, cutoff, dtype)
            out["h_last0"] = st["h_last"]
            ho, hl = [], []
            for c in range(chunks):
                st, outs = sc.update_ref(sd, st, new_ids[c], layers, T, trans, cutoff, dtype)
                ho.append(torch.stack(outs))
                hl.append(st["h_last"])
            out.update({"h_out": torch.stack(ho), "h_last": torch.stack(hl),
                        "win_tail": torch.stack([s["ctx_ln"][:, T - L:] for s in st["layers"]]),
                        "ctx_sum": torch.stack([s["ctx_sum"] for s in st["layers"]])})
            return out

        again, ref64 = restate(torch.float32), restate(torch.float64)
    for k, v64 in ref64.items():
        assert rel_err(again[k].numpy(), rec[k].numpy()) <= 4e-6, (name, k, rel_err(again[k].numpy(), rec[k].numpy()))
        e = rel_err(rec[k].numpy(), v64.numpy())
        assert e <= TOL_ACT / 4, (name, k, e)
        rec["ref_err_" + k] = np.float64(e)
    print(name, {k[8:]: f"{float(v):.1e}" for k, v in rec.items() if k.startswith("ref_err_")})
    rec.update({"ids": ids, "new_ids": new_ids, "seq_len": np.int64(T), "kernel_len": np.int64(K),
                "d_model": np.int64(C), "n_layers": np.int64(layers), "chunk": np.int64(chunk),
                "transition_bins": np.int64(trans), "cutoff": np.int64(-1 if cutoff is None else cutoff)})
    for k, v in sd.items():
        rec["sd." + k] = v
    save(name, rec)


if __name__ == "__main__":
    only = sys.argv[1:]
    cases = [("X01_stream_2x48x32_k8_c4", 2, 48, 8, 32, 4, 2, 14, None, 32),       # 56 rows turn the 48-slot ring
             ("X02_stream_1x64x36_k16_c16", 1, 64, 16, 36, 16, 2, 5, None, 32),    # Vec<4> with idle lanes
             ("X03_stream_3x40x6_k5_c1", 3, 40, 5, 6, 1, 1, 45, None, 32),         # a token at a time, C % 4 != 0
             ("X04_stream_1x256x260_k128_c16", 1, 256, 128, 260, 16, 1, 3, None, 32),   # L = 143, two register chunks
             ("X05_stream_cutoff20_2x48x32", 2, 48, 8, 32, 4, 2, 14, 20, 4)]       # X01 under a cutoff, transition 4
    for c in cases:
        if not only or any(c[0].startswith(p) for p in only):
            stream_case(*c)
