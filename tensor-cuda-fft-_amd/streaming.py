"""Chunk generation with an exact overlap-save update of the backbone: drop-in for the reference's
scripts/generate_chunked_overlap_save.py (init_layer_states :51-74, overlap_save_block_update :78-176,
update_backbone_chunk :179-206, the sampling loop :259-299).

Per layer and per emitted chunk the reference normalises the chunk, concatenates the whole (1, T, C) window, sums it,
runs an rfft and an irfft of n_fft points x C channels and keeps `chunk` of the n_fft rows.  At inference the filter
spectrum H = k_freq sigmoid(gate_freq) (x cutoff mask) is a constant, and so is h_eff = irfft(H, n_fft).  The product
of spectra is the circular convolution y_pad[m] = sum_j h_eff[(m - j) mod n_fft] x_seg[j] of the L = K - 1 + chunk
segment rows, and the kept rows m = K - 1 + n are a (chunk x L) Toeplitz slice of h_eff,
    y[n] = sum_{j < L} taps[n + L - 1 - j] seg[j],     taps[i] = h_eff[(i - (chunk - 1)) mod n_fft],  i < K + 2 chunk - 2
-- negative lags, the wrap of the gated (non-compact) h_eff the reference's FFT includes, among them.

The window lives in a ring (Bt, T, C) that is never copied, with pos (Bt) int32 = the slot of the oldest row in device
memory and the window sum as a compensated fp32 pair (hi, lo).  On a ROCm device one chunk step of a layer is
smx_stream_push -> sigmoid(gate_ctx(pooled)) -> smx_stream_conv -> the FFN's linears: a linear chain with no host
synchronisation, so `update_backbone_chunk` can be captured in a `torch.cuda.graph`.  CPU tensors, `native=False` and
shapes outside smx_stream_supported run the same Toeplitz form in torch on the same ring layout.  The state and both
launches are fp32: a backbone in any other dtype is refused with a TypeError before anything is enqueued.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _lib
from .fixed_spectral import FixedSpectralBlock, cutoff_mask, next_pow2
from .functional import _call, _ptr, _stream, sample_bytes


def stream_taps(block: FixedSpectralBlock, n_fft: int, chunk: int, cutoff=None) -> torch.Tensor:
    """The K + 2 chunk - 2 taps of `block` for chunks of `chunk` rows: taps[i] = h_eff[(i - (chunk - 1)) mod n_fft],
    h_eff = irfft(rfft(zero-pad(kernel), n_fft) sigmoid(gate_freq_logits) cutoff_mask, n_fft).  Built once per
    generation; on a ROCm device by the library's own response and inverse transform."""
    K = block.kernel_len
    fb = n_fft // 2 + 1
    if K + 2 * chunk - 2 > n_fft:
        raise ValueError(f"K + 2 chunk - 2 = {K + 2 * chunk - 2} lags do not fit a period of n_fft = {n_fft}")
    kernel, gate = block.kernel.detach(), block.gate_freq_logits.detach()
    mask = cutoff_mask(cutoff, fb, block.transition_bins, kernel.device)
    if kernel.is_cuda and kernel.dtype == torch.float32 and gate.dtype == torch.float32:
        from .functional import conv_response, irfft
        h_re, h_im = conv_response(kernel, gate, mask, n_fft)
        spec = torch.complex(h_re, h_im).view(1, fb, 1).expand(1, fb, 2).contiguous()    # (a channel pair)
        h_eff = irfft(spec, n_fft)[0, :, 0]
    else:
        k = torch.zeros(n_fft, dtype=torch.float64, device=kernel.device)
        k[:K] = kernel.double()
        H = torch.fft.rfft(k) * torch.sigmoid(gate[:fb].double())
        if mask is not None:
            H = H * mask.double()
        h_eff = torch.fft.irfft(H, n=n_fft).float()
    idx = (torch.arange(K + 2 * chunk - 2, device=kernel.device) - (chunk - 1)) % n_fft
    return h_eff[idx].contiguous()


class LayerStream:
    """The streaming state of one FixedSpectralBlock: ring (Bt, T, C) of LayerNorm outputs, sum (Bt, 2, C) = (hi, lo)
    of the window sum, pos (Bt) int32 = slot of the oldest row, taps (K + 2 chunk - 2)."""

    def __init__(self, ring, sum, pos, taps, kernel_len, chunk):
        self.ring, self.sum, self.pos, self.taps = ring, sum, pos, taps
        self.kernel_len, self.chunk = int(kernel_len), int(chunk)
        L = self.kernel_len - 1 + self.chunk
        n = torch.arange(self.chunk, device=taps.device).unsqueeze(1)
        j = torch.arange(L, device=taps.device).unsqueeze(0)
        self.toeplitz = taps[n + (L - 1) - j].contiguous()                # (chunk, L): the torch path's matrix

    def window(self) -> torch.Tensor:
        """The window in chronological order, (Bt, T, C)."""
        Bt, T, C = self.ring.shape
        idx = (self.pos.long().unsqueeze(1) + torch.arange(T, device=self.ring.device)) % T
        return self.ring.gather(1, idx.unsqueeze(-1).expand(-1, -1, C))

    def pooled(self) -> torch.Tensor:
        """The window mean (Bt, C) the context gate reads."""
        return (self.sum[:, 0] + self.sum[:, 1]) / float(self.ring.shape[1])

    def clone(self) -> "LayerStream":
        return LayerStream(self.ring.clone(), self.sum.clone(), self.pos.clone(), self.taps, self.kernel_len, self.chunk)


class StreamStates:
    """h_last (Bt, C) = ln_f of the newest row, and one LayerStream per block.  `states["h_last"]` and
    `states["layers"]` read as in the reference's loop."""

    def __init__(self, h_last, layers: List[LayerStream], chunk: int, native: bool):
        self.h_last, self.layers, self.chunk, self.native = h_last, layers, int(chunk), bool(native)

    def __getitem__(self, key):
        if key not in ("h_last", "layers"):
            raise KeyError(key)
        return getattr(self, key)

    def clone(self) -> "StreamStates":
        return StreamStates(self.h_last.clone(), [s.clone() for s in self.layers], self.chunk, self.native)


def _require_f32_backbone(backbone) -> None:
    """The streaming state and both launches are fp32: a backbone in another dtype is refused before anything is
    enqueued (the kernels would read its 2-byte or 8-byte rows as floats)."""
    for name, p in backbone.named_parameters():
        if p.dtype != torch.float32:
            raise TypeError(f"chunk streaming needs an fp32 backbone, {name} is {p.dtype} (call .float() on the model)")


def _native_ok(native: bool, h: torch.Tensor, T: int, K: int, C: int, chunk: int) -> bool:
    return bool(native and h.is_cuda and h.dtype == torch.float32
                and _lib.lib().smx_stream_supported(T, K, C, chunk))


def _split_sum(x: torch.Tensor) -> torch.Tensor:
    """(Bt, 2, C) fp32 pair (hi, lo) of the fp64 sum of x (Bt, T, C) over T."""
    s = x.double().sum(dim=1)
    hi = s.float()
    return torch.stack((hi, (s - hi.double()).float()), dim=1).contiguous()


@torch.no_grad()
def init_layer_states(backbone, x_ids: torch.Tensor, chunk: int, cutoff=None, native: bool = True) -> StreamStates:
    """Fill the per-layer rings from one ordinary forward over the context window x_ids (Bt, T) (reference :51-74, any
    batch size).  T must be the blocks' seq_len (init and the updates then share one transform length), the backbone
    fp32.  Only FixedSpectralBlock layers stream: any other block raises TypeError."""
    for blk in backbone.blocks:
        if not isinstance(blk, FixedSpectralBlock):
            raise TypeError(f"only FixedSpectralBlock layers stream, got {type(blk).__name__}")
    _require_f32_backbone(backbone)
    chunk = int(chunk)
    Bt, T = x_ids.shape
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    h = backbone.embed(x_ids)
    layers = []
    ok = True
    for blk in backbone.blocks:
        K = blk.kernel_len
        if K - 1 + chunk > T:
            raise ValueError(f"the overlap-save segment K - 1 + chunk = {K - 1 + chunk} is longer than the window T = {T}")
        if T != blk.seq_len:                                              # init and the updates share one n_fft
            raise ValueError(f"the context window has {T} ids, the blocks were built for seq_len = {blk.seq_len}")
        n_fft = next_pow2(blk.seq_len + K - 1)                            # the transform the block was trained with
        ok = ok and _native_ok(native, h, T, K, h.shape[2], chunk)
        ring = blk.ln(h).contiguous()
        layers.append(LayerStream(ring, _split_sum(ring), torch.zeros(Bt, dtype=torch.int32, device=ring.device),
                                  stream_taps(blk, n_fft, chunk, cutoff), K, chunk))
        h = blk(h, cutoff=cutoff)
    h_last = backbone.ln_f(h)[:, -1, :].contiguous()
    return StreamStates(h_last, layers, chunk, ok)


def _dense_f32(t: Optional[torch.Tensor], name: str = "tensor") -> Optional[torch.Tensor]:
    """An fp32 ROCm tensor, contiguous and 16-byte aligned; anything else is refused before a pointer is taken."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor on a ROCm device, got "
                        f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}"
                        f"{' on ' + str(t.device) if isinstance(t, torch.Tensor) else ''}")
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _state(name: str, t, dtype, shape=None) -> None:
    """ring / sum / pos are updated in place: they are checked, never copied."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous {dtype} tensor on a ROCm device")
    if shape is not None and tuple(t.shape) != shape:
        raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")


def stream_push(h: torch.Tensor, ln: torch.nn.LayerNorm, ring: torch.Tensor, sum: torch.Tensor,
                pos: torch.Tensor) -> torch.Tensor:
    """smx_stream_push: ring[b, (pos[b] + n) % T] = ln(h[b, n]) for the chunk h (Bt, chunk, C), the window sum (hi, lo)
    and pos advanced in place; returns pooled (Bt, C) = the new window mean.  fp32 tensors on a ROCm device."""
    _state("ring", ring, torch.float32)
    Bt, T, C = ring.shape
    _state("sum", sum, torch.float32, (Bt, 2, C))
    _state("pos", pos, torch.int32, (Bt,))
    h = _dense_f32(h, "h")
    if h.dim() != 3 or h.shape[0] != Bt or h.shape[2] != C:
        raise ValueError(f"h must be ({Bt}, chunk, {C}), got {tuple(h.shape)}")
    pooled = torch.empty((Bt, C), dtype=torch.float32, device=h.device)
    w, b = _dense_f32(ln.weight, "ln.weight"), _dense_f32(ln.bias, "ln.bias")
    _call(h.device, "smx_stream_push", h.data_ptr(), _ptr(w), _ptr(b), ln.eps, ring.data_ptr(), sum.data_ptr(),
          pos.data_ptr(), pooled.data_ptr(), Bt, T, C, h.shape[1], _stream(h.device))
    return pooled


def stream_conv(h: torch.Tensor, ring: torch.Tensor, pos: torch.Tensor, taps: torch.Tensor, scale: torch.Tensor,
                ffn_ln: torch.nn.LayerNorm, kernel_len: int):
    """smx_stream_conv: (h_out, ff_in) with h_out = h + scale * (the Toeplitz slice of taps applied to the last
    K - 1 + chunk ring rows) and ff_in = ffn_ln(h_out); pos already advanced by stream_push."""
    _state("ring", ring, torch.float32)
    Bt, T, C = ring.shape
    _state("pos", pos, torch.int32, (Bt,))
    h, scale, taps = _dense_f32(h, "h"), _dense_f32(scale, "scale"), _dense_f32(taps, "taps")
    if h.dim() != 3 or h.shape[0] != Bt or h.shape[2] != C or tuple(scale.shape) != (Bt, C):
        raise ValueError(f"h must be ({Bt}, chunk, {C}) and scale ({Bt}, {C})")
    if taps.numel() != int(kernel_len) + 2 * h.shape[1] - 2:
        raise ValueError(f"taps must hold K + 2 chunk - 2 = {int(kernel_len) + 2 * h.shape[1] - 2} floats")
    w, b = _dense_f32(ffn_ln.weight, "ffn_ln.weight"), _dense_f32(ffn_ln.bias, "ffn_ln.bias")
    h_out, ff_in = torch.empty_like(h), torch.empty_like(h)
    _call(h.device, "smx_stream_conv", h.data_ptr(), ring.data_ptr(), pos.data_ptr(), taps.data_ptr(), scale.data_ptr(),
          _ptr(w), _ptr(b), ffn_ln.eps, h_out.data_ptr(), ff_in.data_ptr(), Bt, T, int(kernel_len), C, h.shape[1],
          _stream(h.device))
    return h_out, ff_in


def _step_native(blk: FixedSpectralBlock, st: LayerStream, h: torch.Tensor) -> torch.Tensor:
    pooled = stream_push(h, blk.ln, st.ring, st.sum, st.pos)                        # reference :101-115
    scale = torch.sigmoid(blk.gate_ctx(pooled)) * blk.gain                          # :116, gain :158
    h_out, ff_in = stream_conv(h, st.ring, st.pos, st.taps, scale, blk.ffn_ln, st.kernel_len)   # :118-172
    return h_out + blk.ffn(ff_in)                                                   # :173


def _step_torch(blk: FixedSpectralBlock, st: LayerStream, h: torch.Tensor) -> torch.Tensor:
    """The same step on the same ring layout in torch (no host synchronisation either)."""
    Bt, T, C = st.ring.shape
    chunk, K = st.chunk, st.kernel_len
    L = K - 1 + chunk
    dev = h.device
    ln_chunk = blk.ln(h).float()
    idx = (st.pos.long().unsqueeze(1) + torch.arange(chunk, device=dev)) % T
    gi = idx.unsqueeze(-1).expand(-1, -1, C)
    d = (ln_chunk - st.ring.gather(1, gi)).sum(dim=1)
    st.ring.scatter_(1, gi, ln_chunk)
    hi, lo = st.sum[:, 0], st.sum[:, 1]
    s = hi + d                                                            # (hi, lo) += d, two-sum
    bb = s - hi
    l2 = lo + ((hi - (s - bb)) + (d - bb))
    h2 = s + l2
    l3 = l2 - (h2 - s)
    st.sum[:, 0].copy_(h2)
    st.sum[:, 1].copy_(l3)
    pooled = (h2 + l3) / float(T)
    st.pos.copy_((st.pos + chunk) % T)
    scale = torch.sigmoid(blk.gate_ctx(pooled)) * blk.gain
    sidx = (st.pos.long().unsqueeze(1) - L + torch.arange(L, device=dev)) % T
    seg = st.ring.gather(1, sidx.unsqueeze(-1).expand(-1, -1, C))         # (Bt, L, C)
    h_out = h + scale.unsqueeze(1) * torch.matmul(st.toeplitz, seg)
    return h_out + blk.ffn(blk.ffn_ln(h_out))


def _chunk_ids(new_ids, Bt: int, chunk: int, device) -> torch.Tensor:
    if isinstance(new_ids, torch.Tensor):
        ids = new_ids
        if ids.is_floating_point() or ids.is_complex():
            raise TypeError("new_ids must be an integer tensor")
    else:
        ids = torch.tensor(new_ids, dtype=torch.long, device=device)
        if ids.dim() == 1:
            ids = ids.unsqueeze(0)                                        # the reference's list of ints: one batch row
    if tuple(ids.shape) != (Bt, chunk):
        raise ValueError(f"new_ids must be ({Bt}, {chunk}) = (batch rows, chunk), got {tuple(ids.shape)}")
    return ids


@torch.no_grad()
def update_backbone_chunk(backbone, states: StreamStates, new_ids, trace: Optional[list] = None) -> StreamStates:
    """Advance the backbone state by one chunk of byte ids (reference :179-206): a list of ints as in the reference
    (one batch row) or a (Bt, chunk) integer tensor.  The states are updated in place and returned.  `trace`, if a
    list, receives each layer's output (Bt, chunk, C)."""
    Bt = states.h_last.shape[0]
    ids = _chunk_ids(new_ids, Bt, states.chunk, states.h_last.device)
    h = backbone.embed(ids)
    step = _step_native if states.native else _step_torch
    for blk, st in zip(backbone.blocks, states.layers):
        h = step(blk, st, h)
        if trace is not None:
            trace.append(h)
    states.h_last.copy_(backbone.ln_f(h)[:, -1, :])
    return states


def _sample_chunk(logits: torch.Tensor, recent: torch.Tensor, temperature: float, top_p: float, rep: float,
                  generator) -> torch.Tensor:
    """logits (chunk, 256) -> (chunk) sampled bytes: repetition penalty over the `recent` ids (reference :285-286),
    temperature, nucleus (:39-48: the longest sorted prefix whose mass stays <= top_p, at least one), multinomial."""
    l = logits.float()
    seen = torch.zeros(l.shape[1], dtype=torch.bool, device=l.device)
    seen[recent] = True
    l = torch.where(seen.unsqueeze(0), l / rep, l) / temperature
    sl, si = torch.sort(l, dim=-1, descending=True)
    keep = torch.cumsum(torch.softmax(sl, dim=-1), dim=-1) <= top_p
    keep[:, 0] = True
    masked = torch.full_like(l, -float("inf")).scatter_(1, si, torch.where(keep, sl, torch.full_like(sl, -float("inf"))))
    return torch.multinomial(torch.softmax(masked, dim=-1), 1, generator=generator).squeeze(1).clamp_(0, 255)


def _native_chunk_step(model, states: StreamStates, win: torch.Tensor, new: torch.Tensor, T: int, temperature: float,
                       top_p: float, rep: float, generator, update: bool) -> None:
    """One whole chunk step on static tensors, capturable as it stands: the EMA scan over the window, ema_proj and head,
    torch.rand, the sampler, the window's shift-and-append and the backbone update.  win (1, max(T, 256)) int64 ends
    with the T ids of the window; new (chunk) int64 receives the chunk."""
    chunk, W = model.chunk, win.shape[1]
    last = states.h_last
    if model.use_ema and T // model.ema_chunk_len > 0:
        state = model.ema.scan_tokens(win[:, W - T:], model.ema_chunk_len)
        last = last + model.ema_proj(torch.view_as_real(state).reshape(1, -1).to(last.dtype))
    logits = model.head(last.float()).view(chunk, 256)
    u = torch.rand(chunk, dtype=torch.float32, device=win.device, generator=generator)
    new.copy_(sample_bytes(logits, win[0, W - 256:], u, temperature=temperature, top_p=top_p, repetition_penalty=rep))
    win.copy_(torch.cat((win[:, chunk:], new.unsqueeze(0)), dim=1))
    if update:
        update_backbone_chunk(model.backbone, states, new.unsqueeze(0))


def _generate_native(model, states: StreamStates, buf: torch.Tensor, T: int, n_chunks: int, temperature: float,
                     top_p: float, rep: float, generator, use_graph: bool) -> None:
    """generate_chunked's loop with sampler="native": fills buf[0, T:].  The torch sampler penalises the last 256 ids of
    the text, which is shorter than that while T + c chunk < 256: the static window is then padded on the left with
    the text's first id -- a duplicate changes no byte's presence, and only presence is penalised here."""
    chunk, dev = model.chunk, buf.device
    W = max(T, 256)
    win = torch.cat((buf[:, :1].repeat(1, W - T), buf[:, :T]), dim=1).contiguous()
    new = torch.zeros(chunk, dtype=torch.long, device=dev)
    step = lambda update: _native_chunk_step(model, states, win, new, T, temperature, top_p, rep, generator, update)
    graph = None
    for c in range(n_chunks):
        if use_graph and dev.type == "cuda" and c > 0:                    # chunk 0 ran eagerly: everything is warm
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                if generator is not None:
                    graph.register_generator_state(generator)
                with torch.cuda.graph(graph):
                    step(True)
            graph.replay()
        else:
            step(c + 1 < n_chunks)                                        # nothing reads the state after the last chunk
        buf[0, T + c * chunk:T + (c + 1) * chunk].copy_(new)              # asynchronous, on the stream of the step


@torch.no_grad()
def generate_chunked(model, prompt: bytes, n_chunks: int, temperature: float = 0.9, top_p: float = 0.9,
                     rep: float = 1.15, generator=None, use_graph: bool = False, native: bool = True,
                     sampler: str = "torch") -> bytes:
    """Sample n_chunks chunks of model.chunk bytes after `prompt` (reference :259-299).  The window is the prompt
    padded on the left with spaces to seq_len (or its last seq_len bytes); the result holds that window and the
    generated bytes, as the reference's `generated` list.  Everything stays on the device until the end.
    use_graph=True captures the backbone update once (after an eager first chunk) and replays it.
    sampler="torch" (the default) draws with about a dozen eager torch ops and torch.multinomial between two replays.
    sampler="native" draws with functional.sample_bytes from torch.rand uniforms (one launch on a ROCm device; another
    random stream than multinomial's), and use_graph=True then captures the WHOLE step once -- EMA scan over a static
    window, ema_proj and head, torch.rand, the sampler, the window's shift-and-append, the backbone update -- and
    replays it: between two replays there is only the asynchronous copy of the chunk's ids into the output buffer, and
    apart from the capture itself no host synchronisation before the final read.  Note: with the native sampler
    top_p >= 1 means no nucleus step; the torch sampler still applies `cdf <= 1` there (and may drop a tail that
    rounding lifts above 1)."""
    if sampler not in ("torch", "native"):
        raise ValueError(f"sampler must be 'torch' or 'native', got {sampler!r}")
    backbone, chunk = model.backbone, model.chunk
    dev = backbone.embed.weight.device
    T = int(backbone.cfg.seq_len)
    ctx = list(bytes(prompt)) or [32]
    init = [32] * (T - len(ctx)) + ctx if len(ctx) < T else ctx[-T:]
    buf = torch.empty((1, T + n_chunks * chunk), dtype=torch.long, device=dev)
    buf[0, :T] = torch.tensor(init, dtype=torch.long, device=dev)
    states = init_layer_states(backbone, buf[:, :T], chunk, native=native)
    if sampler == "native":
        _generate_native(model, states, buf, T, n_chunks, temperature, top_p, rep, generator, use_graph)
        return bytes(buf[0].tolist())
    graph, static_ids = None, torch.zeros((1, chunk), dtype=torch.long, device=dev)
    for c in range(n_chunks):
        n = T + c * chunk
        last = states.h_last
        if model.use_ema and T // model.ema_chunk_len > 0:                # as ChunkLM.forward, over the current window
            state = model.ema.scan_tokens(buf[:, n - T:n], model.ema_chunk_len)
            last = last + model.ema_proj(torch.view_as_real(state).reshape(1, -1).to(last.dtype))
        logits = model.head(last.float()).view(chunk, 256)
        new = _sample_chunk(logits, buf[0, max(0, n - 256):n], temperature, top_p, rep, generator)
        buf[0, n:n + chunk] = new
        if c + 1 == n_chunks:
            break                                                         # nothing reads the state after the last chunk
        if use_graph and dev.type == "cuda":
            static_ids.copy_(new.unsqueeze(0))
            if graph is None and c > 0:                                   # chunk 0 ran eagerly: everything is warm
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    update_backbone_chunk(backbone, states, static_ids)
            if graph is not None:
                graph.replay()
                continue
        update_backbone_chunk(backbone, states, new.unsqueeze(0))
    return bytes(buf[0].tolist())
