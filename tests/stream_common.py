"""Shared by the chunk-generation tests and tests/golden/make_golden_stream.py: a restatement of the reference's op
sequence (fft_lm/train_fixed_full.py:497-563 the block, :606-618 the backbone; scripts/generate_chunked_overlap_save.py
:51-74 init, :78-176 the overlap-save block update, :179-206 the backbone update) in plain torch at ANY precision and
any batch size -- the reference pins fp32 and asserts one batch row -- working on a state_dict of tensors; plus the
parameter distributions and the model builder of the fixtures.  Nothing here imports the package under test or the
reference."""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def mask_ref(cutoff, fbins, trans, dtype=torch.float32):
    """1 up to cutoff - trans, half a cosine down to cutoff, 0 from cutoff on (reference :540-551); None: nothing cut."""
    if cutoff is None:
        return None
    ci = min(int(cutoff), fbins)
    if ci >= fbins:
        return None
    tr = min(int(max(1, trans)), ci)
    m = torch.ones(fbins, dtype=dtype)
    if tr > 0:
        m[ci - tr:ci] = 0.5 * (1.0 + torch.cos(math.pi * torch.linspace(0, 1, steps=tr, dtype=dtype)))
    m[ci:] = 0.0
    return m


def _ln(x, p, name):
    return F.layer_norm(x, x.shape[-1:], p[name + ".weight"], p[name + ".bias"], 1e-5)


def _lin(x, p, name):
    return x @ p[name + ".weight"].T + p[name + ".bias"]


def _ffn(x, p):
    return _lin(F.gelu(_lin(x, p, "ffn.0")), p, "ffn.3")


def _block(sd, i, dtype):
    pre = f"blocks.{i}."
    return {k[len(pre):]: v.to(dtype) for k, v in sd.items() if k.startswith(pre)}


def _response(p, n_fft, trans, cutoff, dtype):
    """k_freq sigmoid(gate_freq) mask, (n_fft // 2 + 1) complex."""
    fb = n_fft // 2 + 1
    k = torch.zeros(n_fft, dtype=dtype)
    K = p["kernel"].shape[0]
    k[:K] = p["kernel"]
    H = torch.fft.rfft(k) * torch.sigmoid(p["gate_freq_logits"][:fb])
    m = mask_ref(cutoff, fb, trans, dtype)
    return H if m is None else H * m


def block_forward_ref(p, x, trans, cutoff=None):
    """The whole block on x (B, T, C) (reference :497-563), dropout off."""
    B, T, C = x.shape
    h = _ln(x, p, "ln")
    n_fft = next_pow2(T + p["kernel"].shape[0] - 1)
    g_ctx = torch.sigmoid(_lin(h.mean(dim=1), p, "gate_ctx"))
    yf = torch.fft.rfft(F.pad(h, (0, 0, 0, n_fft - T)), dim=1) * _response(p, n_fft, trans, cutoff, x.dtype).view(1, -1, 1)
    y = torch.fft.irfft(yf * p["gain"].view(1, 1, -1) * g_ctx.unsqueeze(1), n=n_fft, dim=1)[:, :T]
    x = x + y
    return x + _ffn(_ln(x, p, "ffn_ln"), p)


def hidden_ref(sd, ids, n_layers, trans, cutoff=None, dtype=torch.float64):
    h = sd["embed.weight"].to(dtype)[ids]
    for i in range(n_layers):
        h = block_forward_ref(_block(sd, i, dtype), h, trans, cutoff)
    return _ln(h, {k: v.to(dtype) for k, v in sd.items() if k.startswith("ln_f.")}, "ln_f")


def init_ref(sd, ids, n_layers, trans, cutoff=None, dtype=torch.float64):
    """Reference :51-74: per layer the window of LayerNorm outputs and its sum; h_last."""
    h = sd["embed.weight"].to(dtype)[ids]
    layers = []
    for i in range(n_layers):
        p = _block(sd, i, dtype)
        ln_in = _ln(h, p, "ln")
        layers.append({"ctx_ln": ln_in, "ctx_sum": ln_in.sum(dim=1)})
        h = block_forward_ref(p, h, trans, cutoff)
    h = _ln(h, {k: v.to(dtype) for k, v in sd.items() if k.startswith("ln_f.")}, "ln_f")
    return {"h_last": h[:, -1], "layers": layers}


def block_update_ref(p, st, h_chunk, n_fft, trans, cutoff=None):
    """Reference :78-176 for h_chunk (B, chunk, C): slide the window, pooled gate, overlap-save through the n_fft-point
    transform pair, residual and FFN."""
    K = p["kernel"].shape[0]
    n = h_chunk.shape[1]
    ln_chunk = _ln(h_chunk, p, "ln")
    ctx = torch.cat([st["ctx_ln"][:, n:], ln_chunk], dim=1)
    ctx_sum = ctx.sum(dim=1)
    g_ctx = torch.sigmoid(_lin(ctx_sum / float(ctx.shape[1]), p, "gate_ctx"))
    seg = ctx[:, ctx.shape[1] - (K - 1 + n):]
    xf = torch.fft.rfft(F.pad(seg, (0, 0, 0, n_fft - seg.shape[1])), dim=1)
    yf = xf * _response(p, n_fft, trans, cutoff, h_chunk.dtype).view(1, -1, 1) * p["gain"].view(1, 1, -1) * g_ctx.unsqueeze(1)
    y = torch.fft.irfft(yf, n=n_fft, dim=1)[:, K - 1:K - 1 + n]
    h_out = h_chunk + y
    return h_out + _ffn(_ln(h_out, p, "ffn_ln"), p), {"ctx_ln": ctx, "ctx_sum": ctx_sum}


def update_ref(sd, states, new_ids, n_layers, seq_len, trans, cutoff=None, dtype=torch.float64):
    """Reference :179-206 for new_ids (B, chunk); returns (states, [each layer's output])."""
    h = sd["embed.weight"].to(dtype)[new_ids]
    outs = []
    for i in range(n_layers):
        p = _block(sd, i, dtype)
        n_fft = next_pow2(seq_len + p["kernel"].shape[0] - 1)
        h, states["layers"][i] = block_update_ref(p, states["layers"][i], h, n_fft, trans, cutoff)
        outs.append(h)
    h = _ln(h, {k: v.to(dtype) for k, v in sd.items() if k.startswith("ln_f.")}, "ln_f")
    states["h_last"] = h[:, -1]
    return states, outs


def randomize(model, gen):
    """Every parameter of a FixedSpectralLM (the reference's or the package's) redrawn, so that no term of the update is
    near its initial identity: kernel N(0, 0.3), gain N(1, 0.3), gate_freq_logits N(0.5, 1), gate_ctx.weight N(0, 0.2),
    gate_ctx.bias N(0.5, 0.5), LayerNorm weights N(1, 0.2) and biases N(0, 0.2), FFN weights and biases N(0, 0.1),
    embedding N(0, 1)."""
    with torch.no_grad():
        for name, q in model.named_parameters():
            leaf = name.split(".")[-1]
            r = torch.randn(q.shape, generator=gen)
            if name == "embed.weight":
                q.copy_(r)
            elif leaf == "kernel":
                q.copy_(0.3 * r)
            elif leaf == "gain":
                q.copy_(1.0 + 0.3 * r)
            elif leaf == "gate_freq_logits":
                q.copy_(0.5 + r)
            elif ".gate_ctx." in name:
                q.copy_(0.2 * r if leaf == "weight" else 0.5 + 0.5 * r)
            elif ".ffn." in name:
                q.copy_(0.1 * r)
            elif ".ln." in name or ".ffn_ln." in name or name.startswith("ln_f."):
                q.copy_(1.0 + 0.2 * r if leaf == "weight" else 0.2 * r)
            else:
                raise KeyError(name)


def lm_config(seq_len, kernel_len, d_model, n_layers, trans):
    return SimpleNamespace(vocab_size=256, d_model=int(d_model), n_layers=int(n_layers), seq_len=int(seq_len),
                           kernel_len=int(kernel_len), jpeg_transition=int(trans), bicameral=False,
                           frequency_native=False)


def fixture_config(z):
    return lm_config(z["seq_len"], z["kernel_len"], z["d_model"], z["n_layers"], z["transition_bins"])


def fixture_sd(z):
    return {k[3:]: t(v) for k, v in z.items() if k.startswith("sd.")}


def fixture_cutoff(z):
    return None if int(z["cutoff"]) < 0 else int(z["cutoff"])


def t(a, device=None):
    out = torch.from_numpy(np.ascontiguousarray(a))
    return out if device is None else out.to(device)
