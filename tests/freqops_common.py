"""The formulas of fft_tensor/frequency_ops.py in plain torch at the precision of their inputs: what the goldens of
tests/golden/make_golden_freqops.py are checked against in fp32, and -- evaluated on complex128 copies on the CPU -- the
yardstick of the GPU tests."""
import torch


def attention_ref(q, k, v, temperature=1.0):
    """(B, H, N, D) complex: softmax over n of mean_d(|q conj(k)| / temperature), times v"""
    s = (q * k.conj()).abs().div(temperature).mean(-1)
    return torch.softmax(s, -1)[..., None] * v


def merge_heads(t):
    """(B, H, N, D) -> (B, N, H D)"""
    B, H, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * D)


def split_heads(t, heads):
    """(B, N, H hd) -> the (B, H, N, hd) view"""
    B, N, D = t.shape
    return t.reshape(B, N, heads, D // heads).permute(0, 2, 1, 3)


def layernorm_ref(z, eps=1e-5):
    """last axis: (|z| - mean) / (unbiased std + eps) at the phase of z, the phase of 0 being 0"""
    m = z.abs()
    n = (m - m.mean(-1, keepdim=True)) / (m.std(-1, keepdim=True) + eps)
    return n * torch.polar(torch.ones_like(m), torch.angle(z))


def layer_ref(x, wq, wk, wv, wo, heads):
    """FrequencyTransformerLayer.forward: x (B, N, D), four (D, D) weights"""
    a = attention_ref(split_heads(x @ wq, heads), split_heads(x @ wk, heads), split_heads(x @ wv, heads))
    return merge_heads(a) @ wo


def relu_ref(z):
    return torch.polar(torch.relu(z.abs()), torch.angle(z))


def circulant_ref(x, w_freq):
    """x (B, M, K) real; w_freq (D_out, K) -> x @ w.T, else (K, N) -> x @ w, w = Re(ifft(w_freq, last axis))"""
    w = torch.fft.ifft(w_freq, dim=-1).real
    return x @ (w.T if w_freq.shape[1] == x.shape[2] else w)


def wide(t):
    """a CPU copy at double precision (complex128 / float64)"""
    t = t.detach().cpu()
    return t.to(torch.complex128) if t.is_complex() else t.double() if t.is_floating_point() else t


def crandn(gen, *shape):
    return torch.complex(torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen))
