"""Autograd glue between torch tensors and the C ABI (include/smx.h).

PyTorch is plumbing here: device memory, streams, autograd bookkeeping.  All arithmetic of the
hot path runs in libsmx.so's HIP kernels on torch's current stream.
"""
from __future__ import annotations

import ctypes
import functools
import math
import warnings
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _under_forward_options(backward):
    """Autograd runs backward on ITS OWN thread, where the scoped plan options of the forward call
    (`with _lib.options(...)`, thread-local) are not in force: forward and backward of one node would plan
    differently -- other kernels, another workspace layout for the workspace forward hands over.  Every Function
    below notes the options its forward ran under (ctx.smx_opts) and re-applies them around its backward."""
    @functools.wraps(backward)
    def wrapped(ctx, *args):
        o = getattr(ctx, "smx_opts", None)
        if o is None:
            return backward(ctx, *args)
        with _lib.options(**o):
            return backward(ctx, *args)
    return wrapped


# element type of the streamed x / y / g / grad_x (include/smx.h SMX_IO_*): arithmetic stays fp32 on every one
_IO = {torch.float32: _lib.SMX_IO_F32, torch.bfloat16: _lib.SMX_IO_BF16, torch.float16: _lib.SMX_IO_F16}

_F32 = (torch.float32,)
_C64 = (torch.complex64,)
_ACT = tuple(_IO)
_DTYPE_TEXT = {_ACT: "float32, bfloat16 or float16", _F32: "float32", _C64: "complex64"}
_MIX_PATH = "the MI355X spectral-mixing path has no CPU implementation (move the module and its input to a ROCm device)"
_ANY_PATH = "the MI355X path has no CPU implementation"


def _require(name: str, t, dtypes=_F32, path: str = _MIX_PATH, what: Optional[str] = None, dim: Optional[int] = None,
             typed: bool = True):
    """`t` is a tensor on a ROCm device with one of `dtypes` (None: any; _ACT: the activations spectral_mix takes).
    `path`: the sentence of the device error.  `what` ("a (B, F, C) complex64 tensor"): the ops that describe
    their operand in one sentence raise that one TypeError for a wrong type, device, dtype or rank `dim`.
    typed=False: the ops that never asked whether `t` is a tensor at all -- a non-tensor fails on the first attribute
    read (dtype in the `what` form, is_cuda otherwise) with Python's AttributeError, as it always did there."""
    if what is not None:
        if not ((not typed or isinstance(t, torch.Tensor)) and t.dtype in dtypes and t.is_cuda
                and dim in (None, t.dim())):
            raise TypeError(f"{name} must be {what} on a ROCm device")
        return
    if typed and not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: {path}")
    if dtypes is not None and t.dtype not in dtypes:
        raise TypeError(f"{name} must be {_DTYPE_TEXT[dtypes]}, got {t.dtype}"
                        + ("" if dtypes == _C64 else " (the kernels compute in fp32)"))


def _check_filter(x: torch.Tensor, w_re: torch.Tensor, w_im: torch.Tensor) -> None:
    if w_re.shape != w_im.shape or w_re.dim() != 2 or w_re.shape[0] != x.shape[2]:
        raise ValueError("weights must both be (D, num_filters)")


# bf16 / fp16 activations take two steps, the same for every op that has them: the parameters are read as fp32
# (_fp32_params), and the op runs its native 2-byte rows where the library has them for the shape (_half_native) and
# itself on x.float(), rounded once with .to(x.dtype), everywhere else.
def _fp32_params(x: torch.Tensor, params, required: int = 0) -> tuple:
    """The parameters ((name, tensor or None), ...) beside the activations x, as fp32: they must be fp32 beside an fp32
    x, and fp32 or x's dtype beside a bf16 / fp16 x (`.float()`, so autograd returns their gradients in their own
    dtype).  Beside an fp32 x the first `required` may not be None."""
    half = x.dtype != torch.float32
    for i, (name, t) in enumerate(params):
        if t is None and (half or i >= required):
            continue
        _require(name, t, _ACT if half else _F32)
        if half and t.dtype not in (torch.float32, x.dtype):
            raise TypeError(f"{name} must be float32 or {x.dtype} like x, got {t.dtype}")
    return tuple(t.float() if half and t is not None else t for _, t in params)


def _half_native(x: torch.Tensor, memo: "_Memo", shape: tuple, supported) -> bool:
    """Does the library run this shape with x's 2-byte rows natively?  `supported(*shape, io)`, memoised per shape,
    dtype and plan options."""
    return bool(memo.get(shape + (x.dtype,), lambda: supported(*shape, _IO[x.dtype])))


# One workspace per (device, stream): calls on the same stream are ordered, so reuse is safe.
_ws_cache: dict = {}
# A captured hipGraph replays with the addresses it was captured with.  Workspaces handed out WHILE A STREAM IS
# CAPTURING therefore never come from _ws_cache: they are allocated inside the capture, i.e. from that graph's
# private memory pool, and live exactly as long as the graph does.  Eager workspaces are never referenced by a
# graph, so a buffer that is outgrown simply goes back to the allocator (stream-ordered, same stream).
_WS_CACHE_MAX = 16                      # (device, stream) pairs kept; least recently used goes first


def _stream(dev: torch.device) -> int:
    """The hipStream_t of torch's current stream on `dev` as an integer (the raw C query: torch.cuda.current_stream
    builds a Stream object, ~8 us a call, four calls per eager fwd+bwd: host cost of a small step 0.18-0.22 -> 0.145-0.19 ms,
    A/B in one run, the spread being the shared host CPUs)."""
    return torch._C._cuda_getCurrentRawStream(dev.index)


def _workspace(dev: torch.device, nbytes: int) -> Optional[torch.Tensor]:
    if nbytes == 0:
        return None
    if torch._C._cuda_isCurrentStreamCapturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    key = (dev.index, _stream(dev))
    ws = _ws_cache.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _ws_cache[key] = ws                 # (re)inserted last = most recently used
    while len(_ws_cache) > _WS_CACHE_MAX:
        _ws_cache.pop(next(iter(_ws_cache)))
    return ws


def release_workspaces() -> None:
    """Drop every cached workspace (they return to torch's allocator once the work queued on them is done)."""
    _ws_cache.clear()


class _Memo:
    """Small bounded memo for per-shape answers of the library (plan, workspace size ...).  Keys carry
    _lib.opts_key(), so an entry is only ever found under the plan options it was computed with; the bound keeps
    a variable-length workload from growing it without limit (oldest entries go first)."""

    def __init__(self, cap: int = 512):
        self.cap = cap
        self.d: dict = {}

    def get(self, key, make):
        k = (key, _lib.opts_key())
        v = self.d.get(k)
        if v is None:
            v = self.d[k] = make()
            while len(self.d) > self.cap:
                self.d.pop(next(iter(self.d)))
        return v

    def peek(self, key):
        """the cached value or None, never computing it"""
        return self.d.get((key, _lib.opts_key()))

    def __contains__(self, key):
        return (key, _lib.opts_key()) in self.d

    def __getitem__(self, key):
        return self.d[(key, _lib.opts_key())]

    def clear(self):
        self.d.clear()


_prepared: set = set()
_prepared_epoch = [0]


def _prepare(dev: torch.device, N: int) -> None:
    """smx_prepare(N) once per (device, N): the twiddle tables are uploaded with a blocking copy, which
    must not happen inside a stream capture (the library refuses it there with a clear error).  The set is
    dropped whenever the library evicted tables (smx_tables_epoch), so it never claims more than is on the
    device, and it cannot outgrow the library's own table cache."""
    ep = int(_lib.lib().smx_tables_epoch())
    if ep != _prepared_epoch[0]:
        _prepared.clear()
        _prepared_epoch[0] = ep
    key = (dev.index, int(N))
    if key not in _prepared:
        _call(dev, "smx_prepare", int(N))
        _prepared.add(key)


_ws_bytes_cache = _Memo()


_slow_plan_warned: set = set()


def _note_plan(p, B: int, R: int, D: int, n_fft: int) -> None:
    """One warning per process and reason when a LARGE problem lands on a plan that is far from the streaming
    kernels: DFT products (n_fft % 256 != 0 or odd channel count: ~10x the cost of the neighbouring multiple of
    256) or band groups (more than 512 bins at a tile count the four-step path does not take: x is re-read once
    per 512 bins).  Results are the same on every plan; the reference runs any length at O(N log N)."""
    if B * R * D < (1 << 22):
        return
    if p.path == _lib.SMX_PATH_DIRECT:
        why = ("direct", f"n_fft = {n_fft} is not a multiple of 256 -- nor of 16 with at most 256 bins below the Nyquist "
               f"bin, which streams at about a third of the rate -- (or an odd channel count {D} reached the native op "
               f"directly: spectral_mix pads it): this shape runs "
               f"DFT matrix products, roughly 10x the cost of the neighbouring multiple of 256")
    elif p.groups > 1:
        why = ("groups", f"{p.k} bins at n_fft = {n_fft} (256 x {n_fft // 256} tiles) run as {p.groups} band groups, "
               f"each re-reading the input; tile counts 5..32, 36..64 step 4, 72..128 step 8, 144..256 step 16 "
               f"stream it once")
    else:
        return
    if why[0] not in _slow_plan_warned:
        _slow_plan_warned.add(why[0])
        warnings.warn("tensor_cuda_fft_amd: " + why[1], RuntimeWarning, stacklevel=4)


def _ws_bytes(B: int, N: int, D: int, F: int) -> int:
    """smx_workspace_bytes, memoised per (shape, plan options)."""
    def make():
        _note_plan(_lib.plan(B, N, D, F), B, N, D, N)
        return _lib.workspace_bytes(B, N, D, F)
    return _ws_bytes_cache.get((B, N, D, F), make)


def _dense(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Contiguous and 16-byte aligned (the kernels use 8/16-byte vector accesses): a view that starts at
    an odd element of a larger buffer is copied, everything else is passed through."""
    if t is None:
        return None
    if t.is_complex():
        t = t.resolve_conj()
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _ws_arg(ws: Optional[torch.Tensor]) -> tuple:
    """the (workspace, workspace_bytes) argument pair"""
    return (None, 0) if ws is None else (ws.data_ptr(), ws.numel())


def _call(dev: torch.device, name: str, *args) -> None:
    """One native call on `dev`: the entry point is looked up on the library object by name at every call (tests
    wrap entry points there), a non-zero return code raises SmxError.  The caller places _stream(dev) among `args`."""
    if dev.index == torch.cuda.current_device():
        _lib.check(getattr(_lib.lib(), name)(*args))
    else:                    # (`with torch.cuda.device` is the slow part of a call: only when dev is not current)
        with torch.cuda.device(dev):
            _lib.check(getattr(_lib.lib(), name)(*args))


def _query(name: str, *args, outs: int = 1, unsupported: Optional[int] = None):
    """The size_t out-parameters of a *_workspace_bytes entry: an int, or a tuple for `outs` > 1.  `unsupported`:
    the answer where the entry refuses the shape (default: raise)."""
    out = [ctypes.c_size_t() for _ in range(outs)]
    rc = getattr(_lib.lib(), name)(*args, *(ctypes.byref(o) for o in out))
    if rc != 0 and unsupported is not None:
        return unsupported
    _lib.check(rc)
    return int(out[0].value) if outs == 1 else tuple(int(o.value) for o in out)


def _grad_f32(g: torch.Tensor) -> torch.Tensor:
    """upstream gradient as dense fp32"""
    return _dense(g if g.dtype == torch.float32 else g.float())


def _grad_c64(g: torch.Tensor) -> torch.Tensor:
    """upstream gradient as dense complex64"""
    return _dense(g.to(torch.complex64))


def _grad_slab(D: int, F: int, dev=None, flat: Optional[torch.Tensor] = None):
    """The parameter gradients of one filter live in ONE fp32 buffer [gw_re (D F) | gw_im (D F) | gbias (D)], so a
    single collective reduces all three: (flat, gw_re, gw_im, gbias), the three as views of `flat` (allocated here
    unless given)."""
    if flat is None:
        flat = torch.empty(2 * D * F + D, dtype=torch.float32, device=dev)
    return flat, flat[:D * F], flat[D * F:2 * D * F], flat[2 * D * F:]


def num_bins(N: int, F: int) -> int:
    return min(int(F), int(N) // 2)


class DropoutState:
    """Source of the two 64-bit words (seed, counter) a fused-dropout forward/backward pair shares.

    They are drawn from torch's generator of the device (`torch.randint` on the GPU), so the fused dropout
    follows torch's RNG discipline: `torch.manual_seed` reproduces the masks, a captured hipGraph draws
    fresh words at every replay (torch registers the generator with the graph), and activation
    checkpointing -- which saves and restores the device RNG state around the recomputed forward --
    regenerates the mask of the original forward."""

    def __init__(self, device: torch.device):
        self.device = torch.device(device)

    def next(self) -> torch.Tensor:
        return torch.randint(-(1 << 62), 1 << 62, (2,), dtype=torch.int64, device=self.device)


def _check_p(p: float) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"fused dropout needs 0 <= p < 1, got {p}")
    return p


def _check_dropout(p: float, drop_state) -> float:
    p = _check_p(p)
    if p > 0.0 and drop_state is None:
        raise ValueError("dropout_p > 0 needs a DropoutState")
    return p


_ODD_D_PAD_MIN = 1 << 18        # below this the literal kernels of the direct plan are launch-bound anyway
_io_cache = _Memo()


def forward_raw(x, w_re, w_im, bias, *, conj_w=False, save_spectrum=False, dropout_p=0.0, rng=None,
                pack=None, pack_ready=False, ws=None, io=_lib.SMX_IO_F32):
    """y, xk = smx_forward[_dropout](...).  x (B,N,D) contiguous f32 on GPU; returns xk (B,k,D) c64 or
    None.  rng: the int64[2] device tensor from DropoutState.next() when dropout_p > 0.  pack: (k,D)
    complex64 tensor that receives the packed filter (hand it to backward_raw to skip its packing launch);
    pack_ready=True: `pack` was filled by an earlier call with the same weights, do not pack again.
    io: element type of x and y (SMX_IO_BF16 / SMX_IO_F16: bf16 / fp16 x, 4-byte aligned, on a plan with
    _lib.io_supported; y comes back in x's dtype, xk stays complex64)."""
    B, N, D = x.shape
    F = w_re.shape[1]
    k = num_bins(N, F)
    y = torch.empty_like(x)
    xk = torch.empty((B, k, D), dtype=torch.complex64, device=x.device) if save_spectrum else None
    _prepare(x.device, N)
    if ws is None:
        ws = _workspace(x.device, _ws_bytes(B, N, D, F))
    args = (x.data_ptr(), w_re.data_ptr(), w_im.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(xk), *_ws_arg(ws),
            B, N, D, F, int(bool(conj_w)) | (_lib.SMX_FILTER_PACK_READY if pack_ready else 0), float(dropout_p),
            _ptr(rng), _ptr(pack), _stream(x.device))
    # (2-byte rows through the _io entry, f32 through the f32 entry: the tests tell the routes apart by the call)
    if io:
        _call(x.device, "smx_forward_io", *args, int(io))
    else:
        _call(x.device, "smx_forward_dropout", *args)
    return y, xk


PHASE_SPECTRUM, PHASE_INVERSE, PHASE_PARAMS = _lib.SMX_PHASE_SPECTRUM, _lib.SMX_PHASE_INVERSE, _lib.SMX_PHASE_PARAMS
PHASE_ALL = _lib.SMX_PHASE_ALL


def backward_raw(g, xk, w_re, w_im, *, want_x=True, want_w=True, phases=PHASE_ALL, grad_x=None,
                 flat=None, ws=None, dropout_p=0.0, rng=None, pack=None, io=_lib.SMX_IO_F32):
    """Runs smx_backward.  Returns (grad_x, flat) where flat = [gw_re | gw_im | gbias] fp32.
    `ws`: workspace of an earlier phase (a call made on another stream must not pick that stream's), or the
    workspace the forward call of the same autograd node used.
    io: element type of g and grad_x, as in forward_raw (the parameter gradients stay fp32)."""
    B, N, D = g.shape
    F = w_re.shape[1]
    # with dropout the direct plan stages g * mask in grad_x during the SPECTRUM phase
    if (want_x or (dropout_p > 0.0 and phases & PHASE_SPECTRUM)) and grad_x is None:
        grad_x = torch.empty_like(g)
    gw_re = gw_im = gb = None
    if want_w:
        flat, gw_re, gw_im, gb = _grad_slab(D, F, g.device, flat)
    if ws is None:
        ws = _workspace(g.device, _ws_bytes(B, N, D, F))
    if not want_x:
        phases &= ~PHASE_INVERSE
    _prepare(g.device, N)
    args = (g.data_ptr(), _ptr(xk), w_re.data_ptr(), w_im.data_ptr(), _ptr(grad_x), _ptr(gw_re), _ptr(gw_im), _ptr(gb),
            *_ws_arg(ws), B, N, D, F, phases, float(dropout_p), _ptr(rng), _ptr(pack), _stream(g.device))
    if io:
        _call(g.device, "smx_backward_io", *args, int(io))
    else:
        _call(g.device, "smx_backward_dropout", *args)
    return grad_x, flat


_pack_used_cache = _Memo()


def _new_pack(x: torch.Tensor, w_re: torch.Tensor) -> Optional[torch.Tensor]:
    """(k, D) complex64 buffer for the filter in the kernels' layout (include/smx.h, filter_pack), or None
    where the library would not touch it: small problems, and one band (k <= 128: every workgroup stages its own
    slice of (D, F) through LDS)."""
    B, N, D = x.shape
    F = w_re.shape[1]
    def make():
        p = _lib.plan(B, N, D, F)
        return (p.path == _lib.SMX_PATH_DECIMATED and B * N * D >= 8 * (1 << 20)
                and not (p.bands == 1 and p.groups == 1))
    if not _pack_used_cache.get((B, N, D, F), make):
        return None
    return torch.empty((num_bins(N, F), D), dtype=torch.complex64, device=x.device)


def _phase_split(sync, run, want_x: bool = True):
    """Backward of one node under a gradient sync: SMX_PHASE_SPECTRUM on the main stream, then the parameter-gradient
    reduction (SMX_PHASE_PARAMS, handed to the collective as `pre`) while the grad_x inverse transform
    (SMX_PHASE_INVERSE) runs on the main stream; sync.mode == "fused" folds INVERSE into the first call.
    `run(phases, bufs)` runs those phases into the buffers an earlier phase returned (None: it allocates them) and
    returns them, the gradient slab second.  Returns (bufs, handle); the caller waits on the handle."""
    fused = getattr(sync, "mode", "overlap") == "fused" and want_x
    bufs = run((PHASE_SPECTRUM | PHASE_INVERSE) if fused else PHASE_SPECTRUM, None)
    handle = sync.all_reduce(bufs[1], pre=lambda: run(PHASE_PARAMS, bufs))
    if want_x and not fused:
        run(PHASE_INVERSE, bufs)
    return bufs, handle


class _SpectralMix(torch.autograd.Function):
    """y = real(ifft(pad_k(W * fft(x)[:k]))) + bias, reference fft_tensor/spectral_layers.py:88-116.

    `sync` is None or an object with `.all_reduce(flat, pre)` -> handle-with-wait(); when given and active,
    backward runs in phases around the collective (_phase_split).
    """

    @staticmethod
    def forward(ctx, x, w_re, w_im, bias, sync, dropout_p=0.0, drop_state=None, grad_mode=True):
        ctx.smx_opts = _lib.effective_options()
        # needs_input_grad ignores torch.no_grad(); grad_mode is the caller's torch.is_grad_enabled()
        # (inside forward() it is always off), so inference does not write the spectrum or pack the filter
        needs = grad_mode and any(ctx.needs_input_grad[:4])
        rng = drop_state.next() if dropout_p > 0.0 else None
        pack = _new_pack(x, w_re) if needs else None         # packed filter, reused by backward
        B, N, D = x.shape
        # backward runs on forward's workspace
        ws = _workspace(x.device, _ws_bytes(B, N, D, w_re.shape[1]))
        io = _IO[x.dtype]                                    # bf16 / fp16 x: plans with native 2-byte rows only
        y, xk = forward_raw(x, w_re, w_im, bias, save_spectrum=needs, dropout_p=dropout_p, rng=rng,
                            pack=pack, ws=ws, io=io)
        ctx.io = io
        ctx.io_dtype = x.dtype
        ctx.ws = ws if needs else None
        ctx.sync = sync
        ctx.has_bias = bias is not None
        ctx.drop = (dropout_p, rng)
        ctx.pack = pack
        if needs:
            ctx.save_for_backward(xk, w_re, w_im)
        return y

    @staticmethod
    @once_differentiable
    @_under_forward_options
    def backward(ctx, g):
        xk, w_re, w_im = ctx.saved_tensors
        if g.dtype != ctx.io_dtype:
            g = g.to(ctx.io_dtype)
        g = _dense(g)
        D, F = w_re.shape
        want_x = ctx.needs_input_grad[0]
        want_w = any(ctx.needs_input_grad[1:4])
        sync = ctx.sync if (want_w and ctx.sync is not None and ctx.sync.active()) else None
        dkw = dict(dropout_p=ctx.drop[0], rng=ctx.drop[1], pack=ctx.pack, io=ctx.io)
        if sync is None:
            gx, flat = backward_raw(g, xk, w_re, w_im, want_x=want_x, want_w=want_w, ws=ctx.ws, **dkw)
            if not want_x:
                gx = None
        else:
            def run(phases, bufs):
                inv = phases != PHASE_PARAMS                 # the PARAMS call neither reads nor writes grad_x
                return backward_raw(g, xk, w_re, w_im, want_x=want_x and inv, want_w=True, phases=phases,
                                    grad_x=bufs[0] if bufs and inv else None, flat=bufs[1] if bufs else None,
                                    ws=ctx.ws, **dkw)
            (gx, flat), handle = _phase_split(sync, run, want_x)
            handle.wait()
        if not want_w:
            return gx, None, None, None, None, None, None, None
        _, gwr, gwi, gb = _grad_slab(D, F, flat=flat)
        return gx, gwr.view(D, F), gwi.view(D, F), gb if ctx.has_bias else None, None, None, None, None


def spectral_mix(x: torch.Tensor, weight_real: torch.Tensor, weight_imag: torch.Tensor,
                 bias: Optional[torch.Tensor] = None, sync=None, dropout_p: float = 0.0,
                 drop_state: Optional[DropoutState] = None) -> torch.Tensor:
    """Functional form of SpectralMixingLayer.forward (learnable branch).  dropout_p > 0 applies the
    training-mode dropout of the reference (:118) inside the same launches, masks from `drop_state`.

    x may be fp32, bf16 or fp16; y and grad_x come back in x's dtype.  The parameters are fp32 or x's dtype and are
    read as fp32 (`.float()`, so autograd returns their gradients in their own dtype).  All arithmetic is fp32: the
    result is the fp32 layer's on x.float(), rounded once to x's dtype -- by the kernels' stores where the plan has
    native 2-byte rows (_lib.io_supported), by `.to(dtype)` after the fp32 op everywhere else."""
    _require("x", x, _ACT)
    weight_real, weight_imag, bias = _fp32_params(x, (("weight_real", weight_real), ("weight_imag", weight_imag),
                                                      ("bias", bias)), required=2)
    if x.dim() != 3:
        raise ValueError(f"expected x of shape (B, T, D), got {tuple(x.shape)}")
    _check_filter(x, weight_real, weight_imag)
    B, N, D = x.shape
    half = x.dtype != torch.float32
    # bf16 / fp16 x: native 2-byte rows where the plan has them (the single-launch and residue-split plans with at
    # most 512 bins); everywhere else the up-cast route, which is the same result by construction
    if half and not (x.numel() > 0 and _half_native(x, _io_cache, (B, N, D, weight_real.shape[1]), _lib.io_supported)):
        return spectral_mix(x.float(), weight_real, weight_imag, bias, sync, dropout_p, drop_state).to(x.dtype)
    if x.numel() == 0:
        return torch.empty_like(x)
    dropout_p = _check_dropout(dropout_p, drop_state)
    if not half and D % 2 == 1 and x.numel() >= _ODD_D_PAD_MIN and (
            N % 256 == 0 or (N % 8 == 0 and num_bins(N, weight_real.shape[1]) <= (256 if N % 16 == 0 else 128))):
        # An odd channel count cannot be read as packed float2 pairs, which alone would send the shape to the
        # O(N k) DFT products (~10x).  One zero channel more (its weights and bias zero as well) runs the streaming
        # kernels instead; pad and slice are ordinary differentiable torch ops, so every gradient comes back in
        # the caller's shapes.  The reference handles any D (spectral_layers.py:88); costs one extra copy of x.
        Fp = torch.nn.functional.pad
        y = spectral_mix(Fp(x, (0, 1)), Fp(weight_real, (0, 0, 0, 1)), Fp(weight_imag, (0, 0, 0, 1)),
                         None if bias is None else Fp(bias, (0, 1)), sync, dropout_p, drop_state)
        return y[..., :D]
    F = weight_real.shape[1]
    k = num_bins(N, F)
    if (not half and N % 16 == 8 and D % 2 == 0 and 1 <= k <= 128 and x.numel() >= _ODD_D_PAD_MIN
            and (sync is None or not sync.active())):
        # N = 8 (odd): no sub-transform of the decimated kernels divides it, but the N-point bins ARE the even bins of
        # the 2N-point transform of the zero-padded sequence (w_N^{f n} = w_2N^{2 f n}), and 2N is a multiple of 16:
        # the sixteen-row decimation runs it with rows N .. 2N-1 never read or written.  The filter is expanded to
        # the even bins (odd bins zero; doubled, because the 2N-point inverse divides by 2N) with ordinary
        # differentiable torch ops, so the parameter gradients come back through them in the caller's (D, F) shape.
        def even_bins(w):
            z = torch.zeros_like(w[:, :k])
            return torch.stack((2.0 * w[:, :k], z), dim=2).reshape(D, 2 * k)[:, :2 * k - 1]
        y = spectral_filter(x, even_bins(weight_real), even_bins(weight_imag), bias, n_fft=2 * N, k=2 * k - 1)
        # (training-mode dropout as a separate pass here: the general entry point has no fused one)
        return torch.nn.functional.dropout(y, dropout_p, True) if dropout_p > 0.0 else y
    # _dense: contiguous and 16-byte aligned -- a view with a storage offset is copied before it reaches the library
    return _SpectralMix.apply(_dense(x), _dense(weight_real), _dense(weight_imag), _dense(bias), sync,
                              dropout_p, drop_state, torch.is_grad_enabled())


def block_forward_raw(x, ln_w, ln_b, eps, w_re, w_im, bias, *, save=True, dropout_p=0.0, rng=None,
                      pack=None, ws=None, io=_lib.SMX_IO_F32):
    """y, xk, stats = smx_block_forward(...): y = x + mix(LayerNorm(x)); stats (B,N,2) = (mean, rstd).
    io: element type of x and y (SMX_IO_BF16 / SMX_IO_F16: bf16 / fp16 x, 8-byte aligned, on a shape with
    _lib.block_io_supported; y comes back in x's dtype, xk and stats stay fp32)."""
    B, N, D = x.shape
    F = w_re.shape[1]
    k = num_bins(N, F)
    y = torch.empty_like(x)
    xk = torch.empty((B, k, D), dtype=torch.complex64, device=x.device) if save else None
    stats = torch.empty((B, N, 2), dtype=torch.float32, device=x.device)
    _prepare(x.device, N)
    if ws is None:
        ws = _workspace(x.device, _ws_bytes(B, N, D, F))
    args = (x.data_ptr(), _ptr(ln_w), _ptr(ln_b), float(eps), w_re.data_ptr(), w_im.data_ptr(), _ptr(bias),
            y.data_ptr(), _ptr(xk), stats.data_ptr(), *_ws_arg(ws), B, N, D, F, float(dropout_p), _ptr(rng), _ptr(pack),
            _stream(x.device))
    if io:                                                   # (as forward_raw: 2-byte rows through the _io entry)
        _call(x.device, "smx_block_forward_io", *args, int(io))
    else:
        _call(x.device, "smx_block_forward_dropout", *args)
    return y, xk, stats


def block_backward_raw(g, x, stats, ln_w, xk, w_re, w_im, *, phases=PHASE_ALL, grad_x=None,
                       flat=None, ln_flat=None, ws=None, dropout_p=0.0, rng=None, pack=None, io=_lib.SMX_IO_F32,
                       grad_h=None):
    """Runs smx_block_backward.  Returns (grad_x, flat, ln_flat): flat = [gw_re | gw_im | gbias],
    ln_flat = [g_ln_w | g_ln_b].
    io: element type of g, x and grad_x, as in block_forward_raw (every parameter gradient stays fp32).  A 2-byte io
    needs grad_h, a (B, N, D) fp32 scratch -- the same one for every phase of a phase-split backward; without one it
    comes from torch's allocator for this call."""
    B, N, D = g.shape
    F = w_re.shape[1]
    if grad_x is None:
        grad_x = torch.empty_like(g)
    flat, gw_re, gw_im, gb = _grad_slab(D, F, g.device, flat)
    if ln_flat is None:
        ln_flat = torch.empty(2 * D, dtype=torch.float32, device=g.device)
    if io and grad_h is None:
        grad_h = torch.empty((B, N, D), dtype=torch.float32, device=g.device)
    if ws is None:
        ws = _workspace(g.device, _ws_bytes(B, N, D, F))
    _prepare(g.device, N)
    head = (g.data_ptr(), x.data_ptr(), stats.data_ptr(), _ptr(ln_w), _ptr(xk), w_re.data_ptr(), w_im.data_ptr(),
            grad_x.data_ptr(), ln_flat[:D].data_ptr(), ln_flat[D:].data_ptr(), gw_re.data_ptr(), gw_im.data_ptr(),
            gb.data_ptr())
    tail = (*_ws_arg(ws), B, N, D, F, phases, float(dropout_p), _ptr(rng), _ptr(pack), _stream(g.device))
    if io:
        _call(g.device, "smx_block_backward_io", *head, grad_h.data_ptr(), *tail, int(io))
    else:
        _call(g.device, "smx_block_backward_dropout", *head, *tail)
    return grad_x, flat, ln_flat


class _SpectralBlockMix(torch.autograd.Function):
    """y = x + mix(LayerNorm(x)): first line of SpectralMLPBlock.forward with inactive dropout,
    reference fft_tensor/spectral_layers.py:185.  LayerNorm is applied inside the transform's load
    and the residual inside its store; backward is smx_backward + one LayerNorm-backward pass."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, eps, w_re, w_im, bias, sync, dropout_p=0.0, drop_state=None,
                grad_mode=True):
        ctx.smx_opts = _lib.effective_options()
        needs = grad_mode and any(ctx.needs_input_grad)
        rng = drop_state.next() if dropout_p > 0.0 else None
        pack = _new_pack(x, w_re) if needs else None
        B, N, D = x.shape
        ws = _workspace(x.device, _ws_bytes(B, N, D, w_re.shape[1]))     # shared with backward, see _SpectralMix
        io = _IO[x.dtype]                                    # bf16 / fp16 x: shapes with native 2-byte block rows only
        y, xk, stats = block_forward_raw(x, ln_w, ln_b, eps, w_re, w_im, bias, save=needs,
                                         dropout_p=dropout_p, rng=rng, pack=pack, ws=ws, io=io)
        ctx.io = io
        ctx.io_dtype = x.dtype
        ctx.ws = ws if needs else None
        ctx.sync = sync
        ctx.drop = (dropout_p, rng)
        ctx.pack = pack
        ctx.flags = (ln_w is not None, ln_b is not None, bias is not None)
        if needs:
            ctx.save_for_backward(x, stats, xk, w_re, w_im, ln_w)
        return y

    @staticmethod
    @once_differentiable
    @_under_forward_options
    def backward(ctx, g):
        x, stats, xk, w_re, w_im, ln_w = ctx.saved_tensors
        has_w, has_b, has_bias = ctx.flags
        if g.dtype != ctx.io_dtype:
            g = g.to(ctx.io_dtype)
        g = _dense(g)
        D, F = w_re.shape
        sync = ctx.sync if (ctx.sync is not None and ctx.sync.active()) else None
        dkw = dict(dropout_p=ctx.drop[0], rng=ctx.drop[1], pack=ctx.pack, io=ctx.io)
        if ctx.io and sync is not None:                      # one fp32 grad_h for every phase
            dkw["grad_h"] = torch.empty(g.shape, dtype=torch.float32, device=g.device)
        if sync is None:
            gx, flat, lnf = block_backward_raw(g, x, stats, ln_w, xk, w_re, w_im, ws=ctx.ws, **dkw)
        else:
            def run(phases, bufs):
                gx, flat, lnf = bufs or (None, None, None)
                return block_backward_raw(g, x, stats, ln_w, xk, w_re, w_im, phases=phases, grad_x=gx, flat=flat,
                                          ln_flat=lnf, ws=ctx.ws, **dkw)
            (gx, flat, lnf), handle = _phase_split(sync, run)
            # norm1's weight / bias gradients come out of the LayerNorm backward at the end of the INVERSE
            # phase: a second, tiny (2 D floats) collective, so that every gradient this op returns is
            # already summed over the ranks
            handle2 = sync.all_reduce(lnf) if (has_w or has_b) else None
            handle.wait()
            if handle2 is not None:
                handle2.wait()
        _, gwr, gwi, gb = _grad_slab(D, F, flat=flat)
        return (gx, lnf[:D] if has_w else None, lnf[D:] if has_b else None, None, gwr.view(D, F), gwi.view(D, F),
                gb if has_bias else None, None, None, None, None)


_block_io_cache = _Memo()


def block_supported(D: int) -> bool:
    return bool(_lib.lib().smx_block_supported(int(D)))


def spectral_block_mix(x: torch.Tensor, ln_weight: Optional[torch.Tensor],
                       ln_bias: Optional[torch.Tensor], eps: float, weight_real: torch.Tensor,
                       weight_imag: torch.Tensor, bias: Optional[torch.Tensor] = None,
                       sync=None, dropout_p: float = 0.0,
                       drop_state: Optional[DropoutState] = None) -> torch.Tensor:
    """x + dropout(spectral_mix(layer_norm(x, (D,), ln_weight, ln_bias, eps), weight_real, weight_imag,
    bias), dropout_p).

    x may be fp32, bf16 or fp16; y and grad_x come back in x's dtype.  The parameters are fp32 or x's dtype and are read
    as fp32 (`.float()`, so autograd returns their gradients in their own dtype).  All arithmetic is fp32: the result is
    the fp32 op's on x.float(), rounded once to x's dtype -- by the kernels' stores where the shape has native 2-byte
    block rows (_lib.block_io_supported), by `.to(dtype)` after the fp32 op everywhere else."""
    _require("x", x, _ACT)
    ln_weight, ln_bias, weight_real, weight_imag, bias = _fp32_params(
        x, (("ln_weight", ln_weight), ("ln_bias", ln_bias), ("weight_real", weight_real), ("weight_imag", weight_imag),
            ("bias", bias)))
    if x.dtype != torch.float32:
        # (a shape that is none: not native, and the fp32 call raises what there is to raise)
        shaped = x.dim() == 3 and weight_real.dim() == 2 and x.numel() > 0
        if not (shaped and _half_native(x, _block_io_cache, (*x.shape, weight_real.shape[1]),
                                        _lib.block_io_supported)):
            return spectral_block_mix(x.float(), ln_weight, ln_bias, eps, weight_real, weight_imag, bias, sync,
                                      dropout_p, drop_state).to(x.dtype)
    if x.dim() != 3:
        raise ValueError(f"expected x of shape (B, T, D), got {tuple(x.shape)}")
    D = x.shape[2]
    _check_filter(x, weight_real, weight_imag)
    for name, t in (("ln_weight", ln_weight), ("ln_bias", ln_bias), ("bias", bias)):
        if t is not None and tuple(t.shape) != (D,):
            raise ValueError(f"{name} must have shape ({D},)")
    if x.numel() == 0:
        return torch.empty_like(x)
    dropout_p = _check_dropout(dropout_p, drop_state)
    N = x.shape[1]
    if not block_supported(D) or (x.numel() >= _ODD_D_PAD_MIN and
                                  ((D % 2 == 1 and N % 8 == 0) or (D % 2 == 0 and N % 16 == 8))):
        # rows wider than a wavefront's registers hold (no LayerNorm row kernel takes them), and shapes that only
        # stream through spectral_mix's own routes (one zero channel more; the even bins of twice the length): the
        # block line as the composition it is -- the native block call would refuse the one and run DFT products
        # for the other
        h = torch.nn.functional.layer_norm(x, (D,), ln_weight, ln_bias, eps)
        return x + spectral_mix(h, weight_real, weight_imag, bias, sync, dropout_p, drop_state)
    return _SpectralBlockMix.apply(_dense(x), _dense(ln_weight), _dense(ln_bias), float(eps),
                                   _dense(weight_real), _dense(weight_imag), _dense(bias), sync,
                                   dropout_p, drop_state, torch.is_grad_enabled())


def pruned_rfft(x: torch.Tensor, num_filters: int) -> torch.Tensor:
    """fft(x, dim=1)[:, :k, :] with k = min(num_filters, T//2), without forming the other bins."""
    _require("x", x)
    x = _dense(x)
    B, N, D = x.shape
    k = num_bins(N, num_filters)
    xk = torch.empty((B, k, D), dtype=torch.complex64, device=x.device)
    if k == 0 or x.numel() == 0:
        return xk
    _prepare(x.device, N)
    ws = _workspace(x.device, _ws_bytes(B, N, D, num_filters))
    _call(x.device, "smx_spectrum", x.data_ptr(), xk.data_ptr(), *_ws_arg(ws), B, N, D, num_filters, _stream(x.device))
    return xk


# ---- general shapes: zero-padded rows, explicit bin count, Nyquist bin (include/smx.h, smx_*_ex) -------
def _shape(B, R, D, F, n_fft, k) -> "_lib.smx_shape":
    return _lib.smx_shape(int(B), int(R), int(D), int(F), int(n_fft), int(k))


_ws_ex_cache = _Memo()


def _ws_bytes_ex(key) -> int:
    def make():
        _note_plan(_lib.plan_ex(_shape(*key)), key[0], key[1], key[2], key[4])
        return _lib.workspace_bytes_ex(_shape(*key))
    return _ws_ex_cache.get(key, make)


def hermitian_scale(n_fft: int, k: int, device=None) -> torch.Tensor:
    """(k,) factors that turn the layer's one-sided convention -- y = real(ifft(pad(W X))) -- into
    torch.fft.irfft's: 2 on the bins that have a mirror image, 1 on DC and (even n_fft) on the Nyquist bin."""
    # a constant per (n_fft, k, device): built once on the host and kept (bounded) -- three launches and a
    # host-to-device scalar copy per call otherwise, and that copy is what made PhaseAware / ComplexRoPE steps
    # impossible to capture into a hipGraph.  Callers only read it (out-of-place products).
    dev = torch.device(device) if device is not None else torch.device("cpu")
    key = (int(n_fft), int(k), dev.type, dev.index)

    def make():
        # an ordinary tensor whatever the caller's mode: built under inference_mode it would be an inference tensor,
        # and the training step that multiplies it with a requires-grad filter later could not save it for backward
        with torch.inference_mode(False), torch.no_grad():
            c = torch.full((k,), 2.0, dtype=torch.float32)
            if k > 0:
                c[0] = 1.0
            if n_fft % 2 == 0 and k > n_fft // 2:
                c[n_fft // 2] = 1.0
            return c.to(dev)
    if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        hit = _herm_cache.peek(key)
        if hit is None:           # the host-to-device copy would break the capture, and the tensor would live in
            raise RuntimeError(   # that graph's private pool: build it eagerly first
                f"hermitian_scale({n_fft}, {k}) is not cached on {dev} yet and the stream is being captured: "
                f"run one eager call of this shape before the capture")
        return hit
    return _herm_cache.get(key, make)


_herm_cache = _Memo(64)


_row_scale_ok = _Memo()


def row_scale_supported(key) -> bool:
    """Can the plan of this shape apply a per-(batch row, channel) factor inside its filter stage?"""
    return _row_scale_ok.get(key, lambda: bool(_lib.lib().smx_row_scale_supported(_shape(*key))))


class _SpectralFilter(torch.autograd.Function):
    """y[:, :R] = real(ifft_n(pad_k(W * s * fft_n(zero-pad(x))[:k])))[:, :R] + bias through smx_forward_ex /
    smx_backward_ex: the fused transform for the layer's relatives -- zero-padded causal
    convolution (reference fft_lm/train_fixed_full.py:507-555), full one-sided spectra incl. Nyquist
    (spectral_enhancements.py:147-164, complex_rope.py:207-216).  s = row_scale (B, D) or None."""

    @staticmethod
    def forward(ctx, x, w_re, w_im, bias, row_scale, n_fft, k, grad_mode):
        ctx.smx_opts = _lib.effective_options()
        B, R, D = x.shape
        F = w_re.shape[1]
        key = (B, R, D, F, n_fft, k)
        needs = grad_mode and any(ctx.needs_input_grad[:5])
        y = torch.empty_like(x)
        xk = torch.empty((B, k, D), dtype=torch.complex64, device=x.device) if needs else None
        _prepare(x.device, n_fft)
        ws = _workspace(x.device, _ws_bytes_ex(key))
        _call(x.device, "smx_forward_ex", _shape(*key), x.data_ptr(), w_re.data_ptr(), w_im.data_ptr(), _ptr(bias),
              y.data_ptr(), _ptr(xk), *_ws_arg(ws), 0, None, _ptr(row_scale), _stream(x.device))
        ctx.key = key
        ctx.has_bias = bias is not None
        if needs:
            ctx.save_for_backward(xk, w_re, w_im, row_scale)
        return y

    @staticmethod
    @once_differentiable
    @_under_forward_options
    def backward(ctx, g):
        xk, w_re, w_im, row_scale = ctx.saved_tensors
        B, R, D, F, n_fft, k = ctx.key
        g = _grad_f32(g)
        want_x = ctx.needs_input_grad[0]
        want_w = any(ctx.needs_input_grad[1:4])
        want_s = row_scale is not None and ctx.needs_input_grad[4]
        gx = torch.empty_like(g) if want_x else None
        gwr = gwi = gb = None
        if want_w:
            _, gwr, gwi, gb = _grad_slab(D, F, g.device)
        gs = torch.empty((B, D), dtype=torch.float32, device=g.device) if want_s else None
        ws = _workspace(g.device, _ws_bytes_ex(ctx.key))
        phases = PHASE_ALL if want_x else (PHASE_SPECTRUM | PHASE_PARAMS)
        _call(g.device, "smx_backward_ex", _shape(*ctx.key), g.data_ptr(), _ptr(xk), w_re.data_ptr(), w_im.data_ptr(),
              _ptr(gx), _ptr(gwr), _ptr(gwi), _ptr(gb), *_ws_arg(ws), phases, None, _ptr(row_scale), _ptr(gs),
              _stream(g.device))
        if want_w:
            gwr, gwi, gb = gwr.view(D, F), gwi.view(D, F), gb if ctx.has_bias else None
        return gx, gwr, gwi, gb, gs, None, None, None


def spectral_filter(x: torch.Tensor, weight_real: torch.Tensor, weight_imag: torch.Tensor,
                    bias: Optional[torch.Tensor] = None, *, n_fft: Optional[int] = None,
                    k: Optional[int] = None, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """General form of spectral_mix: x (B, rows, D) is zero-padded to n_fft (default rows), the first k
    bins (default min(F, n_fft // 2), at most n_fft // 2 + 1) are multiplied by W = weight_real + i
    weight_imag (D, F) and the real part of the inverse transform is cropped back to `rows`.  One-sided
    convention as in the layer; multiply W by hermitian_scale() for torch.fft.irfft semantics.
    row_scale (B, D): an extra real factor per (batch row, channel) on the filter -- a gate that depends on
    the batch row -- applied inside the native filter stage where the plan allows (row_scale_supported),
    as a multiply of the output otherwise; differentiable either way."""
    _require("x", x)
    _require("weight_real", weight_real)
    _require("weight_imag", weight_imag)
    if bias is not None:
        _require("bias", bias)
    if x.dim() != 3:
        raise ValueError(f"expected x of shape (B, T, D), got {tuple(x.shape)}")
    B, R, D = x.shape
    _check_filter(x, weight_real, weight_imag)
    F = weight_real.shape[1]
    n_fft = R if n_fft is None else int(n_fft)
    if n_fft < R:
        raise ValueError(f"n_fft={n_fft} is shorter than the sequence ({R})")
    k = min(F, n_fft // 2) if k is None else int(k)
    if not 0 <= k <= min(F, n_fft // 2 + 1):
        raise ValueError(f"k={k} must be in [0, min(F, n_fft // 2 + 1)] = [0, {min(F, n_fft // 2 + 1)}]")
    if row_scale is not None:
        _require("row_scale", row_scale)
        if tuple(row_scale.shape) != (B, D):
            raise ValueError(f"row_scale must be (B, D) = ({B}, {D}), got {tuple(row_scale.shape)}")
        if bias is not None:
            raise ValueError("row_scale and bias together are not defined (the factor is on the filter)")
    if x.numel() == 0:
        return torch.empty_like(x)
    post = None
    if row_scale is not None and not row_scale_supported((B, R, D, F, n_fft, k)):
        post, row_scale = row_scale, None
    y = _SpectralFilter.apply(_dense(x), _dense(weight_real), _dense(weight_imag), _dense(bias),
                              _dense(row_scale), n_fft, k, torch.is_grad_enabled())
    return y if post is None else y * post.unsqueeze(1)


def _rfft_raw(x: torch.Tensor, n_fft: int, k: int, scale: float = 1.0, hermitian: bool = False) -> torch.Tensor:
    """scale * c_f * rfft(x, n_fft, dim=1)[:, :k] (include/smx.h, smx_rfft_ex); no autograd."""
    B, R, D = x.shape
    xk = torch.empty((B, k, D), dtype=torch.complex64, device=x.device)
    if k == 0 or x.numel() == 0:
        return xk
    key = (B, R, D, max(k, 1), n_fft, k)
    _prepare(x.device, n_fft)
    ws = _workspace(x.device, _ws_bytes_ex(key))
    _call(x.device, "smx_rfft_ex", _shape(*key), x.data_ptr(), xk.data_ptr(), float(scale), int(hermitian),
          *_ws_arg(ws), _stream(x.device))
    return xk


def _irfft_raw(spec: torch.Tensor, n_fft: int, rows: int, scale: float, hermitian: bool) -> torch.Tensor:
    """scale * sum_f c_f Re(spec[:, f] e^{+2 pi i f n / n_fft}), n < rows (smx_irfft_ex); no autograd."""
    B, k, D = spec.shape
    y = torch.empty((B, rows, D), dtype=torch.float32, device=spec.device)
    if y.numel() == 0:
        return y
    key = (B, rows, D, max(k, 1), n_fft, k)
    _prepare(spec.device, n_fft)
    ws = _workspace(spec.device, _ws_bytes_ex(key))
    _call(spec.device, "smx_irfft_ex", _shape(*key), spec.data_ptr(), y.data_ptr(), float(scale), int(hermitian),
          *_ws_arg(ws), _stream(spec.device))
    return y


def _check_bins(R: int, n_fft: int, k: int) -> None:
    if n_fft < R or not 0 <= k <= n_fft // 2 + 1:
        raise ValueError(f"need rows <= n_fft and 0 <= k <= n_fft // 2 + 1 (rows={R}, n_fft={n_fft}, k={k})")


def rfft_bins(x: torch.Tensor, k: Optional[int] = None, n_fft: Optional[int] = None) -> torch.Tensor:
    """torch.fft.rfft(x, n=n_fft, dim=1)[:, :k, :] (default: every bin, k = n_fft // 2 + 1) without forming
    the others; no autograd (functional.rfft is the differentiable form)."""
    _require("x", x)
    x = _dense(x.detach())
    R = x.shape[1]
    n_fft = R if n_fft is None else int(n_fft)
    k = n_fft // 2 + 1 if k is None else int(k)
    _check_bins(R, n_fft, k)
    return _rfft_raw(x, n_fft, k)


class _RFFT(torch.autograd.Function):
    """The transform pair of the blocks that work on the spectrum between the transforms (reference
    fft_lm/frequency_native.py:316-317 and :355-356, fft_lm/bicameral.py:170-171 and :203-204).
    y_f = sum_n x_n e^{-i theta}  =>  grad_x[n] = Re sum_f grad_y[f] e^{+i theta}: a synthesis with weight one
    on every bin (torch's convention: grad of a complex tensor = dL/dRe + i dL/dIm)."""

    @staticmethod
    def forward(ctx, x, n_fft, k):
        ctx.smx_opts = _lib.effective_options()
        ctx.dims = (x.shape[1], n_fft)
        return _rfft_raw(x, n_fft, k)

    @staticmethod
    @once_differentiable
    @_under_forward_options
    def backward(ctx, g):
        R, n_fft = ctx.dims
        return _irfft_raw(_dense(g), n_fft, R, 1.0, False), None, None


class _IRFFT(torch.autograd.Function):
    """y[n] = (1/N) sum_f c_f Re(Y_f e^{+i theta})  =>  grad_Y[f] = (c_f / N) rfft(grad_y)[f] (zero-padded rows)."""

    @staticmethod
    def forward(ctx, spec, n_fft, rows):
        ctx.smx_opts = _lib.effective_options()
        ctx.dims = (spec.shape[1], n_fft)
        return _irfft_raw(spec, n_fft, rows, 1.0 / n_fft, True)

    @staticmethod
    @once_differentiable
    @_under_forward_options
    def backward(ctx, g):
        k, n_fft = ctx.dims
        return _rfft_raw(_dense(g), n_fft, k, 1.0 / n_fft, True), None, None


def rfft(x: torch.Tensor, n: Optional[int] = None, k: Optional[int] = None) -> torch.Tensor:
    """torch.fft.rfft(x, n=n, dim=1)[:, :k] of a real (B, rows, D) tensor, rows <= n (zero-padded), with autograd.
    Default k = n // 2 + 1 (every bin)."""
    _require("x", x)
    R = x.shape[1]
    n = R if n is None else int(n)
    k = n // 2 + 1 if k is None else int(k)
    _check_bins(R, n, k)
    return _RFFT.apply(_dense(x), n, k)


def irfft(spec: torch.Tensor, n: Optional[int] = None, rows: Optional[int] = None) -> torch.Tensor:
    """torch.fft.irfft(spec, n=n, dim=1)[:, :rows] of a (B, k, D) complex64 spectrum (bins >= k read as zero,
    as torch pads), with autograd.  Default n = 2 (k - 1), rows = n."""
    _require("spec", spec, _C64, _ANY_PATH, typed=False)
    if spec.dim() != 3:
        raise ValueError(f"spec: expected (B, bins, D), got {tuple(spec.shape)}")
    k = spec.shape[1]
    n = 2 * (k - 1) if n is None else int(n)
    rows = n if rows is None else int(rows)
    if n < 1:
        raise ValueError(f"n must be positive, got {n}")
    if k > n // 2 + 1:                       # torch.fft.irfft trims a longer input
        spec, k = spec[:, :n // 2 + 1], n // 2 + 1
    _check_bins(rows, n, k)
    return _IRFFT.apply(_dense(spec), n, rows)


class _SeqFFT(torch.autograd.Function):
    """torch.fft.fft(z, dim=1) of a COMPLEX (B, N, D) tensor (reference frequency_ops.py:188-204,
    FrequencyAttention.fnet_attention).  A complex channel IS the packed pair the kernels transform: the
    tensor is handed over as real (B, N, 2 D), the one-sided spectra of the real and imaginary parts come
    back from one native pass and are recombined, Z[f] = A[f] + i B[f], Z[N-f] = conj(A[f]) + i conj(B[f]).
    Backward of an unnormalised DFT is the same transform: grad_z = conj(fft(conj(grad_Z)))."""

    @staticmethod
    def forward(ctx, z):
        ctx.smx_opts = _lib.effective_options()
        return seq_fft_raw(z)

    @staticmethod
    @once_differentiable
    @_under_forward_options
    def backward(ctx, g):
        return seq_fft_raw(_dense(g).conj().resolve_conj()).conj().resolve_conj()


_cfft_native = _Memo()


def seq_fft_raw(z: torch.Tensor) -> torch.Tensor:
    _require("z", z, _C64, _ANY_PATH, typed=False)
    if z.dim() != 3:
        raise ValueError(f"expected (B, N, D), got {tuple(z.shape)}")
    B, N, D = z.shape
    if z.numel() == 0:
        return torch.empty_like(z)
    # _dense: a lazily conjugated input (seq_fft(x.conj())) is materialised -- torch.fft.fft accepts such
    # tensors, view_as_real does not -- and a misaligned view is copied
    xr = torch.view_as_real(_dense(z)).reshape(B, N, 2 * D)
    key = (B, N, 2 * D, N // 2 + 1, N, N // 2 + 1)
    fs = _cfft_native.get(key, lambda: _query("smx_cfft_workspace_bytes", _shape(*key), unsupported=0))
    if fs:               # the packed spectrum goes straight out: tile spectra + one column pass
        out = torch.empty((B, N, D), dtype=torch.complex64, device=z.device)
        _prepare(z.device, N)
        ws = _workspace(z.device, fs)
        _call(z.device, "smx_cfft_ex", _shape(*key), xr.data_ptr(), out.data_ptr(), *_ws_arg(ws), _stream(z.device))
        return out
    half = rfft_bins(xr, N // 2 + 1, N)                          # (B, N//2+1, 2D): spectra of re / im parts
    A, Bc = half[..., 0::2], half[..., 1::2]
    out = torch.empty((B, N, D), dtype=torch.complex64, device=z.device)
    out[:, :N // 2 + 1] = A + 1j * Bc
    m = (N - 1) // 2                                             # bins 1..m have a distinct mirror image
    if m > 0:
        out[:, N - m:] = torch.flip(A[:, 1:m + 1].conj() + 1j * Bc[:, 1:m + 1].conj(), dims=(1,))
    return out


def seq_fft(z: torch.Tensor) -> torch.Tensor:
    return _SeqFFT.apply(z)


# ---- rank-one filter: fft_lm's causal FFT convolution with its own kernels (include/smx.h, smx_conv_*) -------
_conv_info = _Memo()


def _conv_plan(B: int, R: int, D: int, n_fft: int):
    """(workspace bytes, saved-spectra bytes) when smx_conv_* takes this shape, else None."""
    def make():
        sh = _shape(B, R, D, n_fft // 2 + 1, n_fft, n_fft // 2 + 1)
        if D % 2 == 0 and n_fft % 256 == 0 and _lib.lib().smx_conv_supported(sh):
            return _query("smx_conv_workspace_bytes", sh, outs=2)
        return ()
    v = _conv_info.get((B, R, D, n_fft), make)
    return v if v else None


def conv_supported(B: int, R: int, D: int, n_fft: int) -> bool:
    return _conv_plan(B, R, D, n_fft) is not None


_conv_io_cache = _Memo()


class _RankOneConv(torch.autograd.Function):
    """y[b, n, c] = s[b, c] * irfft(rfft(zero-pad(x[b, :, c]), n_fft) * (h_re + i h_im), n_fft)[n], n < rows
    (reference fft_lm/train_fixed_full.py:507-555) through smx_conv_forward / smx_conv_backward."""

    @staticmethod
    def forward(ctx, x, h_re, h_im, scale, n_fft, grad_mode):
        ctx.smx_opts = _lib.effective_options()
        B, R, D = x.shape
        wsb, saveb = _conv_plan(B, R, D, n_fft)
        needs = grad_mode and any(ctx.needs_input_grad[:4])
        y = torch.empty_like(x)
        xs = torch.empty(saveb, dtype=torch.uint8, device=x.device) if needs else None
        _prepare(x.device, n_fft)
        ws = _workspace(x.device, wsb)
        sh = _shape(B, R, D, n_fft // 2 + 1, n_fft, n_fft // 2 + 1)
        io = ctx.io = _IO[x.dtype]                           # bf16 / fp16 x: the single-launch plan only (rank_one_conv)
        args = (sh, x.data_ptr(), h_re.data_ptr(), h_im.data_ptr(), _ptr(scale), y.data_ptr(), _ptr(xs), *_ws_arg(ws))
        if io:
            _call(x.device, "smx_conv_forward_io", *args, io, _stream(x.device))
        else:
            _call(x.device, "smx_conv_forward", *args, _stream(x.device))
        ctx.dtype = x.dtype
        ctx.n_fft = n_fft
        if needs:
            ctx.save_for_backward(xs, h_re, h_im, scale)
        return y

    @staticmethod
    @once_differentiable
    @_under_forward_options
    def backward(ctx, g):
        xs, h_re, h_im, scale = ctx.saved_tensors
        if g.dtype != ctx.dtype:
            g = g.to(ctx.dtype)
        g = _dense(g)
        B, R, D = g.shape
        n = ctx.n_fft
        wsb, _ = _conv_plan(B, R, D, n)
        gx = torch.empty_like(g)
        fb = n // 2 + 1
        want_h = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gh = torch.empty((2, fb), dtype=torch.float32, device=g.device) if want_h else None
        gs = torch.empty((B, D), dtype=torch.float32, device=g.device) if scale is not None else None
        ws = _workspace(g.device, wsb)
        sh = _shape(B, R, D, n // 2 + 1, n, n // 2 + 1)
        args = (sh, g.data_ptr(), xs.data_ptr(), h_re.data_ptr(), h_im.data_ptr(), _ptr(scale), gx.data_ptr(),
                None if gh is None else gh[0].data_ptr(), None if gh is None else gh[1].data_ptr(), _ptr(gs),
                *_ws_arg(ws))
        if ctx.io:
            _call(g.device, "smx_conv_backward_io", *args, ctx.io, _stream(g.device))
        else:
            _call(g.device, "smx_conv_backward", *args, _stream(g.device))
        return gx, None if gh is None else gh[0], None if gh is None else gh[1], gs, None, None


class _CausalDwConv3(torch.autograd.Function):
    """y[b, t, c] = scale[b, c] (bias[c] + w[c,0] x[t-2] + w[c,1] x[t-1] + w[c,2] x[t] [t <= T-2]) on (B, T, C): the time
    path of BicameralBlock (reference fft_lm/bicameral.py:214-227) through smx_dwconv3_forward / _backward."""

    @staticmethod
    def forward(ctx, x, w, bias, scale):
        B, T, C = x.shape
        y = torch.empty_like(x)
        _call(x.device, "smx_dwconv3_forward", x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(scale), y.data_ptr(), B, T, C,
              _stream(x.device))
        ctx.save_for_backward(x, w, bias, scale)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w, bias, scale = ctx.saved_tensors
        g = _grad_f32(g)
        B, T, C = x.shape
        ws = _workspace(x.device, _query("smx_dwconv3_workspace_bytes", B, T, C))
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        gb = torch.empty_like(bias) if bias is not None and ctx.needs_input_grad[2] else None
        gs = torch.empty_like(scale) if scale is not None and ctx.needs_input_grad[3] else None
        _call(x.device, "smx_dwconv3_backward", g.data_ptr(), x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(scale), _ptr(gx),
              _ptr(gw), _ptr(gb), _ptr(gs), *_ws_arg(ws), B, T, C, _stream(x.device))
        return gx, gw, gb, gs


def causal_dwconv3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                   scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The time path of fft_lm's BicameralBlock (reference fft_lm/bicameral.py:214-227) on the block's own (B, T, C)
    layout: shift right by one and drop the last position, depthwise `nn.Conv1d(C, C, 3, padding=1, groups=C)` with
    `weight` (C, 1, 3) or (C, 3) and `bias` (C), times `scale` (B, C) (the time gate) -- no transposes, one launch;
    differentiable in x, weight, bias and scale (fixed-order sums)."""
    _require("x", x)
    _require("weight", weight)
    if x.dim() != 3:
        raise ValueError(f"expected (B, T, C), got {tuple(x.shape)}")
    B, T, C = x.shape
    if weight.numel() != 3 * C or weight.shape[0] != C:
        raise ValueError(f"weight must be (C, 1, 3) or (C, 3) with C = {C}, got {tuple(weight.shape)}")
    if bias is not None:
        _require("bias", bias)
        if tuple(bias.shape) != (C,):
            raise ValueError(f"bias must be (C,) = ({C},)")
    if scale is not None:
        _require("scale", scale)
        if tuple(scale.shape) != (B, C):
            raise ValueError(f"scale must be (B, C) = ({B}, {C})")
    if x.numel() == 0:
        return torch.empty_like(x)
    return _CausalDwConv3.apply(_dense(x), _dense(weight.reshape(C, 3)), _dense(bias), _dense(scale))


class _SpectralLN(torch.autograd.Function):
    """SpectralLayerNorm (reference fft_lm/frequency_native.py:203-239) through smx_spectral_ln_forward / _backward:
    z (B, F, C) complex64, gamma / beta (F, C).  planar: the result as (2, B, F, C) float32 planes (real, imaginary)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, eps, planar):
        B, Fq, C = z.shape
        out = torch.empty((2, B, Fq, C), dtype=torch.float32, device=z.device) if planar else torch.empty_like(z)
        _call(z.device, "smx_spectral_ln_forward", torch.view_as_real(z).data_ptr(), gamma.data_ptr(), beta.data_ptr(),
              float(eps), (out if planar else torch.view_as_real(out)).data_ptr(), int(planar), B, Fq, C,
              _stream(z.device))
        ctx.eps, ctx.planar = float(eps), bool(planar)
        ctx.save_for_backward(z, gamma, beta)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z, gamma, beta = ctx.saved_tensors
        B, Fq, C = z.shape
        g = _grad_f32(g) if ctx.planar else _grad_c64(g)
        gz = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        gg = torch.empty_like(gamma) if ctx.needs_input_grad[1] else None
        gb = torch.empty_like(beta) if ctx.needs_input_grad[2] else None
        _call(z.device, "smx_spectral_ln_backward", (g if ctx.planar else torch.view_as_real(g)).data_ptr(),
              torch.view_as_real(z).data_ptr(), gamma.data_ptr(), beta.data_ptr(), ctx.eps,
              None if gz is None else torch.view_as_real(gz).data_ptr(), _ptr(gg), _ptr(gb), int(ctx.planar), B, Fq, C,
              _stream(z.device))
        return gz, gg, gb, None, None


class _PlanarCmul(torch.autograd.Function):
    """out = h (f_re + i f_im)[f, c] on (2, B, F, C) planes: PhaseShift between SpectralFFN's Linear layers (reference
    fft_lm/frequency_native.py:62-77, :175) through smx_planar_cmul_*."""

    @staticmethod
    def forward(ctx, h, f_re, f_im):
        _, B, Fq, C = h.shape
        out = torch.empty_like(h)
        _call(h.device, "smx_planar_cmul_forward", h.data_ptr(), f_re.data_ptr(), f_im.data_ptr(), out.data_ptr(), B, Fq, C,
              _stream(h.device))
        ctx.save_for_backward(h, f_re, f_im)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        h, f_re, f_im = ctx.saved_tensors
        _, B, Fq, C = h.shape
        g = _grad_f32(g)
        gh = torch.empty_like(h) if ctx.needs_input_grad[0] else None
        gr = torch.empty_like(f_re) if ctx.needs_input_grad[1] else None
        gi = torch.empty_like(f_im) if ctx.needs_input_grad[2] else None
        _call(h.device, "smx_planar_cmul_backward", g.data_ptr(), h.data_ptr(), f_re.data_ptr(), f_im.data_ptr(), _ptr(gh),
              _ptr(gr), _ptr(gi), B, Fq, C, _stream(h.device))
        return gh, gr, gi


class _AddPlanar(torch.autograd.Function):
    """y = a + (p[0] + i p[1]): a, y complex64 (...), p float32 (2, ...) -- the residual around SpectralFFN (reference
    fft_lm/frequency_native.py:355-356) with the planar result of its second Linear folded in."""

    @staticmethod
    def forward(ctx, a, p):
        y = torch.empty_like(a)
        _call(a.device, "smx_planar_add", torch.view_as_real(a).data_ptr(), p.data_ptr(), torch.view_as_real(y).data_ptr(),
              a.numel(), _stream(a.device))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = _grad_c64(g)
        gp = None
        if ctx.needs_input_grad[1]:
            gp = torch.empty((2,) + tuple(g.shape), dtype=torch.float32, device=g.device)
            _call(g.device, "smx_planar_split", torch.view_as_real(g).data_ptr(), gp.data_ptr(), g.numel(),
                  _stream(g.device))
        return (g if ctx.needs_input_grad[0] else None), gp


class _SpectralGate(torch.autograd.Function):
    """y = ((((x a[f]) u[c]) p[f]) q[b,c]) m[f] on a (B, F, C) complex64 spectrum: the chain between the two transforms of
    fft_lm's twin blocks (reference fft_lm/frequency_native.py:95, :338, :351; fft_lm/bicameral.py:179-186) through
    smx_spectral_gate_*: one launch forward, one backward (+ the tiny products that finish the parameter gradients)."""

    @staticmethod
    def forward(ctx, x, a, u, p, q, m, reference_gain_grad):
        B, Fq, C = x.shape
        y = torch.empty_like(x)
        _call(x.device, "smx_spectral_gate_forward", x.data_ptr(), a.data_ptr(), _ptr(u), _ptr(p), _ptr(q), _ptr(m),
              y.data_ptr(), B, Fq, C, _stream(x.device))
        ctx.reference_gain_grad = bool(reference_gain_grad)
        ctx.save_for_backward(x, a, u, p, q, m)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, a, u, p, q, m = ctx.saved_tensors
        B, Fq, C = x.shape
        g = _grad_c64(g)
        need = ctx.needs_input_grad
        gx = torch.empty_like(x) if need[0] else None
        want_u = u is not None and need[2]
        s1 = torch.empty(Fq, dtype=torch.complex64, device=x.device) if need[1] or (p is not None and need[3]) else None
        plain = want_u and ctx.reference_gain_grad
        rc = (torch.empty(B, C, dtype=torch.float32, device=x.device)
              if (q is not None and need[4]) or (want_u and not plain) else None)
        rp = torch.empty(B, C, dtype=torch.float32, device=x.device) if plain else None
        ws = _workspace(x.device, _query("smx_spectral_gate_workspace_bytes", B, Fq, C))
        _call(x.device, "smx_spectral_gate_backward", g.data_ptr(), x.data_ptr(), a.data_ptr(), _ptr(u), _ptr(p), _ptr(q),
              _ptr(m), _ptr(gx), _ptr(s1), _ptr(rc), _ptr(rp), *_ws_arg(ws), B, Fq, C, _stream(x.device))
        ga = gu = gp = gq = None
        if need[1]:
            ga = s1 if p is None and m is None else s1 * (p if m is None else m if p is None else p * m)      # :111
        if p is not None and need[3]:
            gp = (a.conj() * s1).real
            if m is not None:
                gp = gp * m
        if q is not None and need[4]:
            gq = rc if u is None else rc * u
        if want_u:
            r = rp if plain else rc                       # :115 sums Re(grad x k) -- no conjugate -- for the gain
            gu = (r if q is None else r * q).sum(dim=0)
        return gx, ga, gu, gp, gq, None, None


def spectral_gate(x: torch.Tensor, a: torch.Tensor, u: Optional[torch.Tensor] = None, p: Optional[torch.Tensor] = None,
                  q: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                  reference_gain_grad: bool = False) -> torch.Tensor:
    """`((((x * a[f]) * u[c]) * p[f]) * q[b,c]) * m[f]` for a complex64 spectrum x (B, F, C): a (F) complex64 -- the kernel
    spectrum --, u (C) the per-channel gain, p (F) the frequency gate, q (B, C) the context gate, m (F) the cutoff mask (a
    constant), each optional.  Differentiable in x, a, u, p and q.  `reference_gain_grad=True` gives u the gradient
    `FrequencyConvFunc.backward` writes by hand (reference fft_lm/frequency_native.py:115: `Re(grad * x * k)` summed, no
    conjugate) instead of the autograd one.  The channel count must be even."""
    _require("x", x, _C64, what="a (B, F, C) complex64 tensor", dim=3, typed=False)
    B, Fq, C = x.shape
    if a.dtype != torch.complex64 or tuple(a.shape) != (Fq,):
        raise ValueError(f"a must be complex64 (F,) = ({Fq},), got {a.dtype} {tuple(a.shape)}")
    for name, t, shape in (("u", u, (C,)), ("p", p, (Fq,)), ("q", q, (B, C)), ("m", m, (Fq,))):
        if t is not None:
            _require(name, t)
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    if C % 2:
        raise ValueError(f"spectral_gate takes an even channel count, got {C}")
    if x.numel() == 0:
        return x.clone()
    d = lambda t: None if t is None else _dense(t)
    return _SpectralGate.apply(_dense(x), _dense(a), d(u), d(p), d(q), d(m.detach() if m is not None else None),
                               reference_gain_grad)


@functools.lru_cache(None)
def _mix_ws_bytes() -> int:
    """a constant of the library, asked once"""
    return _query("smx_mix_workspace_bytes")


class _MixPaths(torch.autograd.Function):
    """out = r + w[0] a + w[1] b + c3 c: BicameralBlock's fusion line and residual (reference fft_lm/bicameral.py
    :237-268) through smx_mix_*: one launch each way, the two scalar gradients summed in a fixed order."""

    @staticmethod
    def forward(ctx, r, a, b, c, w, c3):
        out = torch.empty_like(r)
        _call(r.device, "smx_mix_forward", r.data_ptr(), a.data_ptr(), b.data_ptr(), _ptr(c), w.data_ptr(), float(c3),
              out.data_ptr(), r.numel(), _stream(r.device))
        ctx.c3 = float(c3)
        ctx.has_c = c is not None
        ctx.save_for_backward(a, b, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, w = ctx.saved_tensors
        g = _grad_f32(g)
        need = ctx.needs_input_grad
        ga = torch.empty_like(a) if need[1] else None
        gb = torch.empty_like(b) if need[2] else None
        gc = torch.empty_like(a) if ctx.has_c and need[3] else None
        gw = torch.empty_like(w) if need[4] else None
        ws = _workspace(a.device, _mix_ws_bytes())
        _call(a.device, "smx_mix_backward", g.data_ptr(), a.data_ptr(), b.data_ptr(), w.data_ptr(), ctx.c3, _ptr(ga),
              _ptr(gb), _ptr(gc), _ptr(gw), *_ws_arg(ws), a.numel(), _stream(a.device))
        return (g if need[0] else None), ga, gb, gc, gw, None


def mix_paths(r: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: Optional[torch.Tensor], w: torch.Tensor,
              c3: float = 0.1) -> torch.Tensor:
    """`r + w[0] * a + w[1] * b + c3 * c` for float32 tensors of one shape (element count a multiple of 4) and two learned
    scalars `w` (2,) in device memory; differentiable in r, a, b, c and w."""
    for name, t in (("r", r), ("a", a), ("b", b), ("w", w)) + ((("c", c),) if c is not None else ()):
        _require(name, t)
    if a.shape != r.shape or b.shape != r.shape or (c is not None and c.shape != r.shape) or tuple(w.shape) != (2,):
        raise ValueError("mix_paths: r, a, b, c must share one shape and w must be (2,)")
    if r.numel() == 0 or r.numel() % 4:
        raise ValueError(f"mix_paths takes a positive element count that is a multiple of 4, got {r.numel()}")
    return _MixPaths.apply(_dense(r), _dense(a), _dense(b), _dense(c), _dense(w), c3)


def planar_cmul(h: torch.Tensor, f_re: torch.Tensor, f_im: torch.Tensor) -> torch.Tensor:
    """(2, B, F, C) planes times the complex factor (f_re + i f_im)[f, c]."""
    _require("h", h)
    _require("f_re", f_re)
    _require("f_im", f_im)
    if h.dim() != 4 or h.shape[0] != 2 or tuple(f_re.shape) != tuple(h.shape[2:]) or f_re.shape != f_im.shape:
        raise ValueError(f"expected h (2, B, F, C) and factors (F, C), got {tuple(h.shape)}, {tuple(f_re.shape)}")
    return _PlanarCmul.apply(_dense(h), _dense(f_re), _dense(f_im))


def add_planar(a: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """a + (p[0] + i p[1]) for a complex64 `a` and float32 planes p (2, *a.shape)."""
    _require("a", a, _C64, what="a complex64 tensor", typed=False)
    _require("p", p)
    if tuple(p.shape) != (2,) + tuple(a.shape):
        raise ValueError(f"p must be (2, {tuple(a.shape)}), got {tuple(p.shape)}")
    return _AddPlanar.apply(_dense(a), _dense(p))


def spectral_layer_norm_supported(C: int) -> bool:
    return bool(_lib.lib().smx_spectral_ln_supported(int(C)))


def spectral_layer_norm(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                        planar: bool = False) -> torch.Tensor:
    """Magnitudes of z (B, F, C) complex64 normalised across the channels per (batch row, bin), scaled by gamma (F, C),
    shifted by beta (F, C), phases kept (reference fft_lm/frequency_native.py:203-239); differentiable in all three.
    planar: return (2, B, F, C) float32 planes (real, imaginary) instead of a complex tensor."""
    _require("z", z, None, _ANY_PATH, typed=False)
    if z.dtype != torch.complex64 or z.dim() != 3:
        raise TypeError(f"z must be a (B, F, C) complex64 tensor, got {z.dtype} {tuple(z.shape)}")
    _require("gamma", gamma)
    _require("beta", beta)
    B, Fq, C = z.shape
    if tuple(gamma.shape) != (Fq, C) or tuple(beta.shape) != (Fq, C):
        raise ValueError(f"gamma and beta must be (F, C) = ({Fq}, {C})")
    if z.numel() == 0:
        return torch.empty((2,) + tuple(z.shape), device=z.device) if planar else torch.empty_like(z)
    return _SpectralLN.apply(_dense(z), _dense(gamma), _dense(beta), float(eps), bool(planar))


class _PhaseFilter(torch.autograd.Function):
    """(w_re, w_im)[d, f] = c_f m[d] (cos p[d], sin p[d]), f < k: PhaseAwareSpectralMixing's filter (reference
    fft_tensor/spectral_enhancements.py:147-164) in one native launch, its backward in one more."""

    @staticmethod
    def forward(ctx, m, p, k, n_fft):
        D = m.numel()
        w = torch.empty((2, D, k), dtype=torch.float32, device=m.device)
        _call(m.device, "smx_phase_filter", m.data_ptr(), p.data_ptr(), D, k, n_fft, w[0].data_ptr(), w[1].data_ptr(),
              _stream(m.device))
        ctx.k, ctx.n_fft = k, n_fft
        ctx.save_for_backward(m, p)
        return w[0], w[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_re, g_im):
        m, p = ctx.saved_tensors
        D, k = m.numel(), ctx.k
        g_re = torch.zeros((D, k), device=m.device) if g_re is None else _dense(g_re.float())
        g_im = torch.zeros((D, k), device=m.device) if g_im is None else _dense(g_im.float())
        gm = torch.empty_like(m) if ctx.needs_input_grad[0] else None
        gp = torch.empty_like(p) if ctx.needs_input_grad[1] else None
        if gm is not None or gp is not None:
            _call(m.device, "smx_phase_filter_backward", m.data_ptr(), p.data_ptr(), g_re.data_ptr(), g_im.data_ptr(), D, k,
                  ctx.n_fft, k, _ptr(gm), _ptr(gp), _stream(m.device))
        return gm, gp, None, None


def phase_filter(m: torch.Tensor, p: torch.Tensor, k: int, n_fft: int):
    """(w_re, w_im), each (D, k): c_f m[d] exp(i p[d]) with torch.fft.irfft's Hermitian weights c_f."""
    _require("magnitude", m)
    _require("phase", p)
    if m.dim() != 1 or m.shape != p.shape:
        raise ValueError("magnitude and phase must be 1-D tensors of the same length")
    return _PhaseFilter.apply(_dense(m), _dense(p), int(k), int(n_fft))


class _ConvResponse(torch.autograd.Function):
    """H[f] = rfft(zero-pad(kernel), n_fft)[f] * sigmoid(gate_logits[f]) * mask[f] in one native launch
    (reference fft_lm/train_fixed_full.py:511-513, :529, :540-551) -> (Re H, Im H); backward in one more."""

    @staticmethod
    def forward(ctx, kernel, gate_logits, mask, n_fft):
        fb = n_fft // 2 + 1
        h = torch.empty((2, fb), dtype=torch.float32, device=kernel.device)
        _prepare(kernel.device, n_fft)
        _call(kernel.device, "smx_conv_response", n_fft, kernel.numel(), kernel.data_ptr(), _ptr(gate_logits), _ptr(mask),
              h[0].data_ptr(), h[1].data_ptr(), _stream(kernel.device))
        ctx.n_fft = n_fft
        ctx.save_for_backward(kernel, gate_logits, mask)
        return h[0], h[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_re, g_im):
        kernel, logits, mask = ctx.saved_tensors
        n = ctx.n_fft
        fb = n // 2 + 1
        g_re = torch.zeros(fb, device=kernel.device) if g_re is None else _dense(g_re.float())
        g_im = torch.zeros(fb, device=kernel.device) if g_im is None else _dense(g_im.float())
        gk = torch.empty_like(kernel) if ctx.needs_input_grad[0] else None
        gl = torch.empty_like(logits) if (logits is not None and ctx.needs_input_grad[1]) else None
        if gk is not None or gl is not None:
            _call(kernel.device, "smx_conv_response_backward", n, kernel.numel(), 0 if logits is None else logits.numel(),
                  kernel.data_ptr(), _ptr(logits), _ptr(mask), g_re.data_ptr(), g_im.data_ptr(), _ptr(gk), _ptr(gl),
                  _stream(kernel.device))
        return gk, gl, None, None


def conv_response(kernel: torch.Tensor, gate_logits: Optional[torch.Tensor], mask: Optional[torch.Tensor],
                  n_fft: int):
    """(Re H, Im H) of the causal kernel's n_fft-point response times sigmoid(gate_logits) and mask (each may be
    None); gate_logits may be longer than n_fft // 2 + 1 (the reference sizes it for its longest sequence)."""
    _require("kernel", kernel)
    fb = n_fft // 2 + 1
    if gate_logits is not None:
        _require("gate_logits", gate_logits)
        if gate_logits.dim() != 1 or gate_logits.numel() < fb:
            raise ValueError(f"gate_logits needs at least n_fft // 2 + 1 = {fb} entries")
    if mask is not None:
        _require("mask", mask)
        if tuple(mask.shape) != (fb,):
            raise ValueError(f"mask must have n_fft // 2 + 1 = {fb} entries")
    if kernel.dim() != 1 or kernel.numel() > n_fft:
        raise ValueError("kernel must be 1-D with at most n_fft taps")
    return _ConvResponse.apply(_dense(kernel), _dense(gate_logits), _dense(mask), int(n_fft))


def rank_one_conv(x: torch.Tensor, h_re: torch.Tensor, h_im: torch.Tensor,
                  scale: Optional[torch.Tensor], n_fft: int) -> torch.Tensor:
    """Causal / circular convolution of every (batch, channel) column of x (B, rows, D) with the real kernel
    whose one-sided spectrum is h_re + i h_im (n_fft // 2 + 1), times scale[b, c]; needs
    conv_supported(B, rows, D, n_fft).

    x may be fp32, bf16 or fp16; y and grad_x come back in x's dtype, while h_re, h_im and scale stay fp32.  All
    arithmetic is fp32: the result is the fp32 op's on x.float(), rounded once to x's dtype -- by the kernel's stores
    where the plan has native 2-byte rows (_lib.conv_io_supported), by `.to(dtype)` after the fp32 op elsewhere."""
    _require("x", x, _ACT)
    _require("h_re", h_re)
    _require("h_im", h_im)
    B, R, D = x.shape
    fb = n_fft // 2 + 1
    if tuple(h_re.shape) != (fb,) or tuple(h_im.shape) != (fb,):
        raise ValueError(f"h_re / h_im must have n_fft // 2 + 1 = {fb} entries")
    if scale is not None:
        _require("scale", scale)
        if tuple(scale.shape) != (B, D):
            raise ValueError(f"scale must be (B, D) = ({B}, {D})")
    if not conv_supported(B, R, D, n_fft):
        raise ValueError(f"rank_one_conv does not take (B={B}, rows={R}, D={D}, n_fft={n_fft}); use spectral_filter")
    if x.dtype != torch.float32 and not _half_native(x, _conv_io_cache, (B, R, D, n_fft), _lib.conv_io_supported):
        return rank_one_conv(x.float(), h_re, h_im, scale, n_fft).to(x.dtype)
    # _dense: contiguous and 16-byte aligned -- a view with a storage offset is copied before it reaches the library
    return _RankOneConv.apply(_dense(x), _dense(h_re), _dense(h_im), _dense(scale), int(n_fft),
                              torch.is_grad_enabled())


# ---- row lines of EnhancedSpectralBlock (reference fft_tensor/spectral_enhancements.py:278-333), smx_enh.hip -------

@functools.lru_cache(None)
def enh_supported(D: int) -> bool:
    """Even D <= 1024: the row kernels of the enhanced block hold a row (the gate row: 2D) in one wavefront.
    (A property of the library, not of the plan options: remembered per D, not in an options-keyed _Memo.)"""
    return bool(_lib.lib().smx_enh_supported(int(D)))


def _enh_workspace(dev: torch.device, B: int, T: int, D: int) -> torch.Tensor:
    return _workspace(dev, _query("smx_enh_workspace_bytes", B, T, D))


def _grad_buf(t: Optional[torch.Tensor], needed: bool) -> Optional[torch.Tensor]:
    return torch.empty_like(t) if (t is not None and needed) else None


def _g(g: Optional[torch.Tensor], like: torch.Tensor) -> torch.Tensor:
    """An upstream gradient autograd left undefined (output unused) is zero."""
    if g is None:
        return torch.zeros_like(like)
    return _grad_f32(g)


class _RopeNorm(torch.autograd.Function):
    """Line 1 of the block and the norm of line 2 (reference :321, :324):  x1 = x + M1 rope(norm1(x)),
    h2 = norm2(x1), through smx_rope_norm_forward / _backward.  norm = False: the standalone rotation."""

    @staticmethod
    def forward(ctx, x, rot, rot_rows, w1, b1, w2, b2, eps1, eps2, norm, dropout_p, drop_state):
        B, T, D = x.shape
        rng = drop_state.next() if dropout_p > 0.0 else None
        x1 = torch.empty_like(x)
        h2 = torch.empty_like(x) if norm else None
        stats = torch.empty((2, B, T, 2), dtype=torch.float32, device=x.device) if norm else None
        _call(x.device, "smx_rope_norm_forward", x.data_ptr(), rot.data_ptr(), rot_rows, _ptr(w1), _ptr(b1), _ptr(w2),
              _ptr(b2), float(eps1), float(eps2), x1.data_ptr(), _ptr(h2), _ptr(stats), B, T, D, int(norm),
              float(dropout_p), _ptr(rng), _stream(x.device))
        ctx.meta = (rot_rows, norm, dropout_p, rng)
        ctx.save_for_backward(x if norm else None, rot, w1, b1, w2, stats)
        if not norm:
            return x1
        return x1, h2

    @staticmethod
    @once_differentiable
    def backward(ctx, g1, gh2=None):
        x, rot, w1, b1, w2, stats = ctx.saved_tensors
        rot_rows, norm, dropout_p, rng = ctx.meta
        g1 = _g(g1, x) if norm else _grad_f32(g1)
        B, T, D = g1.shape
        nig = ctx.needs_input_grad
        gx = torch.empty_like(g1)
        gw1, gb1, gw2 = _grad_buf(w1, nig[3]), _grad_buf(b1, nig[4]), _grad_buf(w2, nig[5])
        gb2 = torch.empty(D, dtype=torch.float32, device=g1.device) if (norm and nig[6]) else None
        ws = _enh_workspace(g1.device, B, T, D) if norm else None
        gh2 = _g(gh2, g1) if norm else None
        _call(g1.device, "smx_rope_norm_backward", g1.data_ptr(), _ptr(gh2), _ptr(x), rot.data_ptr(), rot_rows, _ptr(w1),
              _ptr(b1), _ptr(w2), _ptr(stats), gx.data_ptr(), _ptr(gw1), _ptr(gb1), _ptr(gw2), _ptr(gb2), *_ws_arg(ws),
              B, T, D, int(norm), float(dropout_p), _ptr(rng), _stream(g1.device))
        return gx, None, None, gw1, gb1, gw2, gb2, None, None, None, None, None


class _ResidualNorm(torch.autograd.Function):
    """The residual of line 2 and norm3 (reference :324, :327): x2 = x1 + M2 p, h3 = norm3(x2)."""

    @staticmethod
    def forward(ctx, x1, p, w3, b3, eps, dropout_p, drop_state):
        B, T, D = x1.shape
        rng = drop_state.next() if dropout_p > 0.0 else None
        x2, h3 = torch.empty_like(x1), torch.empty_like(x1)
        stats = torch.empty((B, T, 2), dtype=torch.float32, device=x1.device)
        _call(x1.device, "smx_residual_norm_forward", x1.data_ptr(), p.data_ptr(), _ptr(w3), _ptr(b3), float(eps),
              x2.data_ptr(), h3.data_ptr(), stats.data_ptr(), B, T, D, float(dropout_p), _ptr(rng), _stream(x1.device))
        ctx.meta = (dropout_p, rng)
        ctx.save_for_backward(x2, w3, b3, stats)
        return x2, h3

    @staticmethod
    @once_differentiable
    def backward(ctx, g2, gh3):
        x2, w3, b3, stats = ctx.saved_tensors
        dropout_p, rng = ctx.meta
        g2, gh3 = _g(g2, x2), _g(gh3, x2)
        B, T, D = x2.shape
        nig = ctx.needs_input_grad
        gx1 = torch.empty_like(x2)
        gp = torch.empty_like(x2) if dropout_p > 0.0 else None      # without dropout grad_p is grad_x1 itself
        gw3, gb3 = _grad_buf(w3, nig[2]), _grad_buf(b3, nig[3])
        ws = _enh_workspace(x2.device, B, T, D)
        _call(x2.device, "smx_residual_norm_backward", g2.data_ptr(), gh3.data_ptr(), x2.data_ptr(), _ptr(w3),
              stats.data_ptr(), gx1.data_ptr(), _ptr(gp), _ptr(gw3), _ptr(gb3), *_ws_arg(ws), B, T, D, float(dropout_p),
              _ptr(rng), _stream(x2.device))
        return gx1, (gp if gp is not None else gx1), gw3, gb3, None, None, None


class _GateBlend(torch.autograd.Function):
    """GatedSpectralUnit after its two Linears, plus the residual of line 3 (reference :105-114, :327):
    [z | vt] = LayerNorm_2D(a),  x3 = x2 + M3 (sigmoid(z) v + (1 - sigmoid(z)) vt)  (x2 None: the unit alone)."""

    @staticmethod
    def forward(ctx, a, v, x2, wg, bg, eps, dropout_p, drop_state):
        B, T, D = v.shape
        rng = drop_state.next() if dropout_p > 0.0 else None
        x3 = torch.empty_like(v)
        stats = torch.empty((B, T, 2), dtype=torch.float32, device=v.device)
        _call(v.device, "smx_gate_blend_forward", a.data_ptr(), v.data_ptr(), _ptr(x2), _ptr(wg), _ptr(bg), float(eps),
              x3.data_ptr(), stats.data_ptr(), B, T, D, float(dropout_p), _ptr(rng), _stream(v.device))
        ctx.meta = (dropout_p, rng)
        ctx.save_for_backward(a, v, wg, bg, stats)
        return x3

    @staticmethod
    @once_differentiable
    def backward(ctx, g3):
        a, v, wg, bg, stats = ctx.saved_tensors
        dropout_p, rng = ctx.meta
        g3 = _g(g3, v)
        B, T, D = v.shape
        nig = ctx.needs_input_grad
        ga, gv = torch.empty_like(a), torch.empty_like(v)
        gwg, gbg = _grad_buf(wg, nig[3]), _grad_buf(bg, nig[4])
        ws = _enh_workspace(v.device, B, T, D)
        _call(v.device, "smx_gate_blend_backward", g3.data_ptr(), a.data_ptr(), v.data_ptr(), _ptr(wg), _ptr(bg),
              stats.data_ptr(), ga.data_ptr(), gv.data_ptr(), _ptr(gwg), _ptr(gbg), *_ws_arg(ws), B, T, D,
              float(dropout_p), _ptr(rng), _stream(v.device))
        return ga, gv, (g3 if nig[2] else None), gwg, gbg, None, None, None


def _rotation_rows(rotation: torch.Tensor, D: int):
    """(float view of the complex64 table with rows of D floats, its row count)."""
    if rotation.dtype != torch.complex64:
        raise TypeError(f"rotation must be complex64, got {rotation.dtype}")
    if rotation.shape[1] != D // 2:
        rotation = rotation[:, :D // 2]
    return _dense(torch.view_as_real(rotation)), int(rotation.shape[0])


def _check_rows(x: torch.Tensor, D: int) -> None:
    _require("x", x)
    if x.dim() != 3 or x.shape[-1] != D:
        raise ValueError(f"expected (B, T, {D}), got {tuple(x.shape)}")
    if not enh_supported(D):
        raise ValueError(f"the enhanced-block row kernels take an even D <= 1024, got {D}")


def rope_rotate(x: torch.Tensor, rotation: torch.Tensor) -> torch.Tensor:
    """RotaryFrequencyEmbedding.forward (reference :47-71): channel pairs of x (B, T, D) as complex numbers times
    rotation[t] ((max_seq_len, >= D/2) complex64), one launch each way."""
    B, T, D = x.shape
    _check_rows(x, D)
    rot, rows = _rotation_rows(rotation, D)
    if T > rows:
        raise RuntimeError(f"sequence length {T} exceeds the rotation table ({rows} positions)")
    return _RopeNorm.apply(_dense(x), rot, rows, None, None, None, None, 0.0, 0.0, False, 0.0, None)


def rope_norm(x: torch.Tensor, rotation: torch.Tensor, w1, b1, w2, b2, eps1: float, eps2: float,
              dropout_p: float = 0.0, drop_state: Optional[DropoutState] = None):
    """(x1, h2) = (x + dropout(rope(LayerNorm(x; w1, b1))), LayerNorm(x1; w2, b2)): line 1 of the block."""
    B, T, D = x.shape
    _check_rows(x, D)
    rot, rows = _rotation_rows(rotation, D)
    if T > rows:
        raise RuntimeError(f"sequence length {T} exceeds the rotation table ({rows} positions)")
    p = _check_p(dropout_p)
    return _RopeNorm.apply(_dense(x), rot, rows, _dense(w1), _dense(b1), _dense(w2), _dense(b2), float(eps1),
                           float(eps2), True, p, drop_state if p > 0.0 else None)


def residual_norm(x1: torch.Tensor, p_in: torch.Tensor, w3, b3, eps: float, dropout_p: float = 0.0,
                  drop_state: Optional[DropoutState] = None):
    """(x2, h3) = (x1 + dropout(p_in), LayerNorm(x2; w3, b3))."""
    B, T, D = x1.shape
    _check_rows(x1, D)
    _check_rows(p_in, D)
    p = _check_p(dropout_p)
    return _ResidualNorm.apply(_dense(x1), _dense(p_in), _dense(w3), _dense(b3), float(eps), p,
                               drop_state if p > 0.0 else None)


def gate_blend(a: torch.Tensor, v: torch.Tensor, x2: Optional[torch.Tensor], wg, bg, eps: float,
               dropout_p: float = 0.0, drop_state: Optional[DropoutState] = None) -> torch.Tensor:
    """x2 + dropout(g v + (1 - g) vt) with [z | vt] = LayerNorm(a; wg, bg) over 2D and g = sigmoid(z) (x2 None:
    the blend alone, GatedSpectralUnit.forward after its Linears)."""
    B, T, D = v.shape
    _check_rows(v, D)
    _require("a", a)
    if tuple(a.shape) != (B, T, 2 * D):
        raise ValueError(f"a must be (B, T, 2D) = ({B}, {T}, {2 * D}), got {tuple(a.shape)}")
    if x2 is not None:
        _check_rows(x2, D)
    p = _check_p(dropout_p)
    return _GateBlend.apply(_dense(a), _dense(v), _dense(x2), _dense(wg), _dense(bg), float(eps), p,
                            drop_state if p > 0.0 else None)


# ---- SpectralEMA: the chunk head's state-space memory as one scan launch (csrc/smx_ema.hip) ---------------------------
EMA_MODES = {"aligned": _lib.SMX_EMA_ALIGNED, "polar": _lib.SMX_EMA_POLAR}


def _ema_mode(mode: str) -> int:
    if mode not in EMA_MODES:
        raise ValueError(f"unknown SpectralEMA mode {mode!r} (expected 'aligned' or 'polar')")
    return EMA_MODES[mode]


def _ema_ws(dev: torch.device, B: int, S: int, F: int):
    return _workspace(dev, _query("smx_ema_workspace_bytes", B, S, F))


class _EmaScan(torch.autograd.Function):
    """Final state of the scan over (B, S, F) complex64 chunks (reference fft_lm/spectral_ssm.py:107-125) through
    smx_ema_scan_forward / _backward.  The forward saves its inputs only: the backward launch reruns the chain."""

    @staticmethod
    def forward(ctx, chunks, rho_logit, theta_raw, init, mode):
        B, S, F = chunks.shape
        out = torch.empty((B, F), dtype=torch.complex64, device=chunks.device)
        _call(chunks.device, "smx_ema_scan_forward", chunks.data_ptr(), _ptr(init), rho_logit.data_ptr(),
              theta_raw.data_ptr(), out.data_ptr(), mode, B, S, F, _stream(chunks.device))
        ctx.mode = mode
        ctx.save_for_backward(chunks, rho_logit, theta_raw, init)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        chunks, rho_logit, theta_raw, init = ctx.saved_tensors
        B, S, F = chunks.shape
        g = _grad_c64(g)
        need = ctx.needs_input_grad
        gx = torch.empty_like(chunks) if need[0] else None
        gr = torch.empty_like(rho_logit) if need[1] else None
        gt = torch.empty_like(theta_raw) if need[2] and ctx.mode == _lib.SMX_EMA_ALIGNED else None
        gi = torch.empty_like(g) if init is not None and need[3] else None
        ws = _ema_ws(g.device, B, S, F)
        _call(g.device, "smx_ema_scan_backward", g.data_ptr(), chunks.data_ptr(), _ptr(init), rho_logit.data_ptr(),
              theta_raw.data_ptr(), _ptr(gx), _ptr(gi), _ptr(gr), _ptr(gt), *_ws_arg(ws), ctx.mode, B, S, F,
              _stream(g.device))
        return gx, gr, gt, gi, None


class _EmaScanTokens(torch.autograd.Function):
    """The same scan with chunk t of row b formed in the kernel from byte tokens (reference fft_lm/chunk_head.py:56-65)
    through smx_ema_tokens_forward / _backward: the (B, S, F) spectrum is never written."""

    @staticmethod
    def forward(ctx, tokens, L, rho_logit, theta_raw, mode):
        B, T = tokens.shape
        out = torch.empty((B, L // 2 + 1), dtype=torch.complex64, device=tokens.device)
        ctx.args = (tokens.data_ptr(), tokens.element_size(), tokens.stride(0))
        _call(tokens.device, "smx_ema_tokens_forward", *ctx.args, None, rho_logit.data_ptr(), theta_raw.data_ptr(),
              out.data_ptr(), mode, B, T, L, _stream(tokens.device))
        ctx.mode, ctx.L = mode, L
        ctx.save_for_backward(tokens, rho_logit, theta_raw)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        tokens, rho_logit, theta_raw = ctx.saved_tensors
        B, T = tokens.shape
        L = ctx.L
        g = _grad_c64(g)
        gr = torch.empty_like(rho_logit) if ctx.needs_input_grad[2] else None
        gt = torch.empty_like(theta_raw) if ctx.needs_input_grad[3] and ctx.mode == _lib.SMX_EMA_ALIGNED else None
        ws = _ema_ws(g.device, B, T // L, L // 2 + 1)
        _call(g.device, "smx_ema_tokens_backward", g.data_ptr(), *ctx.args, None, rho_logit.data_ptr(),
              theta_raw.data_ptr(), None, _ptr(gr), _ptr(gt), *_ws_arg(ws), ctx.mode, B, T, L, _stream(g.device))
        return None, None, gr, gt, None


def _ema_params(F: int, rho_logit: torch.Tensor, theta_raw: torch.Tensor):
    for name, p in (("rho_logit", rho_logit), ("theta_raw", theta_raw)):
        _require(name, p)
        if tuple(p.shape) != (F,):
            raise ValueError(f"{name} must be (F,) = ({F},), got {tuple(p.shape)}")
    return _dense(rho_logit), _dense(theta_raw)


def ema_scan(chunks: torch.Tensor, rho_logit: torch.Tensor, theta_raw: torch.Tensor, mode: str = "aligned",
             init: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Final (B, F) complex64 state of fft_lm's SpectralEMA over `chunks` (B, S, F) complex64 from `init` (B, F)
    (None: zeros): one launch forward, one scan launch and a small fixed-order sum backward; differentiable in chunks,
    rho_logit, theta_raw (None in polar mode, where it takes no part) and init."""
    m = _ema_mode(mode)
    _require("chunks", chunks, _C64, what="a (B, S, F) complex64 tensor", dim=3)
    B, S, F = chunks.shape
    rho_logit, theta_raw = _ema_params(F, rho_logit, theta_raw)
    if init is not None and not (init.is_cuda and init.dtype == torch.complex64 and tuple(init.shape) == (B, F)):
        raise TypeError(f"init must be (B, F) = ({B}, {F}) complex64 on the device of chunks")
    if B == 0:
        return chunks.new_empty((0, F))
    return _EmaScan.apply(_dense(chunks), rho_logit, theta_raw, _dense(init), m)


def _token_rows(tokens: torch.Tensor) -> torch.Tensor:
    """(B, T) tokens as the kernels read them in place -- unit stride along a row, rows at least T elements apart, aligned
    to the element -- else their contiguous copy."""
    if tokens.shape[1] > 1 and tokens.stride(1) != 1 or tokens.stride(0) < tokens.shape[1] \
            or tokens.data_ptr() % tokens.element_size():
        return tokens.contiguous()
    return tokens


def ema_scan_tokens(tokens: torch.Tensor, chunk_len: int, rho_logit: torch.Tensor, theta_raw: torch.Tensor,
                    mode: str = "aligned") -> torch.Tensor:
    """ema_scan over the chunk spectra of byte tokens (B, T), uint8 or int64: chunk t of row b is the
    `chunk_len`-point real DFT of tokens[b, t L : (t + 1) L] / 127.5 - 1, formed inside the scan kernel (2 <= L <= 64;
    bytes past (T // L) L are ignored).  Differentiable in rho_logit and theta_raw (None in polar mode)."""
    m = _ema_mode(mode)
    L = int(chunk_len)
    if not 2 <= L <= 64:
        raise ValueError(f"chunk_len must be in 2..64, got {L}")
    _require("tokens", tokens, (torch.uint8, torch.int64), what="a (B, T) uint8 or int64 tensor", dim=2)
    rho_logit, theta_raw = _ema_params(L // 2 + 1, rho_logit, theta_raw)
    if tokens.shape[0] == 0:
        return torch.empty((0, L // 2 + 1), dtype=torch.complex64, device=tokens.device)
    tokens = _token_rows(tokens)
    return _EmaScanTokens.apply(tokens, L, rho_logit, theta_raw, m)


# ---- word-structure heads of the bicameral trainer: targets and the O-neuron row head (csrc/smx_ema.hip, smx_block.hip) --

def _in_phase_set(v: torch.Tensor) -> torch.Tensor:
    """P = {32..47} u {58..64}: where the phase clock breaks words (reference fft_lm/phase_clock.py:89)."""
    return ((v >= 32) & (v <= 47)) | ((v >= 58) & (v <= 64))


def _in_boundary_set(v: torch.Tensor) -> torch.Tensor:
    """S = P u {91..96} u {123..126} u {10, 13}: what ends a word for the boundary label (reference
    fft_lm/segmentation_head.py:81-92).  The two sets differ on purpose."""
    return _in_phase_set(v) | ((v >= 91) & (v <= 96)) | ((v >= 123) & (v <= 126)) | (v == 10) | (v == 13)


def _word_targets_torch(tokens: torch.Tensor, phase: bool, boundary: bool):
    """The two target functions as a handful of whole-tensor ops (what CPU tokens run): a cummax / cummin pair for the
    word of every position, angles in fp64 rounded once."""
    B, T = tokens.shape
    v = tokens.to(torch.int64)
    ph = bd = None
    if boundary:
        bd = torch.ones((B, T), dtype=torch.float32, device=v.device)
        bd[:, :-1] = _in_boundary_set(v[:, 1:]).to(torch.float32)
    if phase:
        d = _in_phase_set(v)
        idx = torch.arange(T, device=v.device).expand(B, T)
        last = torch.cummax(torch.where(d, idx, torch.full_like(idx, -1)), dim=1).values
        nxt = torch.cummin(torch.where(d, idx, torch.full_like(idx, T)).flip(1), dim=1).values.flip(1)
        start = last + 1
        ang = (idx - start).double() / (nxt - start - 1).clamp(min=1).double() * torch.pi
        ph = torch.stack((torch.cos(ang), torch.sin(ang)), dim=-1).to(torch.float32)
        ph = torch.where(d[..., None], torch.zeros_like(ph), ph)
    return ph, bd


def word_targets(tokens: torch.Tensor, phase: bool = True, boundary: bool = True):
    """(phase, boundary) of byte tokens (B, T), uint8 or int64, each None when not asked for, on the tokens' device:
    phase (B, T, 2) fp32, the phase-clock targets of fft_lm.phase_clock.generate_phase_targets -- position q of a word of
    n bytes at (cos, sin)(pi q / (n - 1)), delimiters at (0, 0) -- and boundary (B, T) fp32, the labels of
    fft_lm.segmentation_head.get_word_boundaries.  On a ROCm device both come from ONE launch with no host
    synchronisation (T <= 65536); CPU tokens take the same functions as whole-tensor torch ops.  Not differentiable."""
    if not (isinstance(tokens, torch.Tensor) and tokens.dtype in (torch.uint8, torch.int64) and tokens.dim() == 2):
        raise TypeError("tokens must be a (B, T) uint8 or int64 tensor")
    if not (phase or boundary):
        raise ValueError("word_targets: neither phase nor boundary asked for")
    B, T = tokens.shape
    dev = tokens.device
    if not tokens.is_cuda or B == 0 or T == 0:
        if B == 0 or T == 0:
            return (torch.zeros((B, T, 2), dtype=torch.float32, device=dev) if phase else None,
                    torch.zeros((B, T), dtype=torch.float32, device=dev) if boundary else None)
        return _word_targets_torch(tokens, phase, boundary)
    tokens = _token_rows(tokens)
    ph = torch.empty((B, T, 2), dtype=torch.float32, device=dev) if phase else None
    bd = torch.empty((B, T), dtype=torch.float32, device=dev) if boundary else None
    _call(dev, "smx_word_targets", tokens.data_ptr(), tokens.element_size(), tokens.stride(0), _ptr(ph), _ptr(bd), B, T,
          _stream(dev))
    return ph, bd


@functools.lru_cache(None)
def head_supported(C: int, O: int) -> bool:
    """O in {1, 2} and C a width of the LayerNorm row kernels.  (A property of the library, remembered per (C, O).)"""
    return bool(_lib.lib().smx_head_supported(int(C), int(O)))


@functools.lru_cache(None)
def _head_ws_bytes(R: int, C: int, O: int) -> int:
    """smx_head_workspace_bytes: a function of the shape alone, remembered per shape (one host call less per step)."""
    return _query("smx_head_workspace_bytes", R, C, O)


class _NarrowHead(torch.autograd.Function):
    """y = h w^T + b over (R, C) rows with O = 1 or 2 outputs (reference fft_lm/phase_clock.py:65,
    fft_lm/segmentation_head.py:55) through smx_head_forward / _backward: only the gradients autograd asks for are formed."""

    @staticmethod
    def forward(ctx, h, w, b):
        R, C = h.shape
        O = w.shape[0]
        y = torch.empty((R, O), dtype=torch.float32, device=h.device)
        _call(h.device, "smx_head_forward", h.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), R, C, O,
              _stream(h.device))
        ctx.has_bias = b is not None
        ctx.save_for_backward(h, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        h, w = ctx.saved_tensors
        R, C = h.shape
        O = w.shape[0]
        nig = ctx.needs_input_grad
        gh = torch.empty_like(h) if nig[0] else None
        gw = torch.empty_like(w) if nig[1] else None
        gb = torch.empty(O, dtype=torch.float32, device=h.device) if ctx.has_bias and nig[2] else None
        if gh is None and gw is None and gb is None:
            return None, None, None
        g = _grad_f32(g)
        ws = _workspace(h.device, _head_ws_bytes(R, C, O))
        _call(h.device, "smx_head_backward", g.data_ptr(), h.data_ptr(), w.data_ptr(), _ptr(gh), _ptr(gw), _ptr(gb),
              *_ws_arg(ws), R, C, O, _stream(h.device))
        return gh, gw, gb


def narrow_head(h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear(h, weight, bias) for a weight of one or two rows: (..., C) -> (..., O).  Native -- one wavefront per
    row, the backward bitwise reproducible -- when h is an fp32 tensor on a ROCm device with fp32 parameters, C is a width
    of the LayerNorm row kernels (head_supported) and autocast is off; F.linear everywhere else (CPU, bf16 / fp16,
    under torch.autocast, other widths)."""
    O, C = weight.shape
    native = (h.is_cuda and h.dtype == torch.float32 and weight.dtype == torch.float32 and weight.device == h.device
              and (bias is None or (bias.dtype == torch.float32 and bias.device == h.device))
              and h.shape[-1] == C and h.numel() > 0 and not torch.is_autocast_enabled() and head_supported(C, O))
    if not native:
        return torch.nn.functional.linear(h, weight, bias)
    y = _NarrowHead.apply(_dense(h.reshape(-1, C)), _dense(weight), _dense(bias))
    return y.view(*h.shape[:-1], O)


# ---- softmax cross-entropy: the losses of the dual head (csrc/smx_block.hip, k_xent_*) ------------------------------------

_XENT_REDUCTION = {"mean": _lib.SMX_XENT_MEAN, "sum": _lib.SMX_XENT_SUM, "none": _lib.SMX_XENT_NONE}


@functools.lru_cache(None)
def _xent_ws_bytes(R: int, V: int) -> int:
    """smx_xent_workspace_bytes: a function of the shape alone, remembered per shape (one host call less per step)."""
    return _query("smx_xent_workspace_bytes", R, V)


def _xent_rows(logits: torch.Tensor):
    """(rows, row_stride): `logits` (..., V) as (R, V) rows the kernels read in place -- a view whose last dimension is
    contiguous and whose rows share one stride of at least V elements -- and a dense copy of anything else."""
    V = logits.shape[-1]
    x = logits.reshape(-1, V)               # a view where the leading dimensions share one stride, a dense copy otherwise
    if (V > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < V) or x.data_ptr() % 4:
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else V)


class _CrossEntropy(torch.autograd.Function):
    """Softmax cross-entropy of (R, V) fp32 rows with int64 targets through smx_xent_forward / _backward: the logits are
    read once per direction, lse (R, 2) -- the pair (row maximum, log-sum-exp relative to it) -- and the count of live rows
    stay on the device, the upstream gradient is read there."""

    @staticmethod
    def forward(ctx, x, row_stride, targets, ignore_index, reduction):
        R, V = x.shape
        n_loss = R if reduction == _lib.SMX_XENT_NONE else 1
        buf = torch.empty(2 * R + 1 + n_loss, dtype=torch.float32, device=x.device)  # lse (R, 2) | count | loss
        ws = _workspace(x.device, _xent_ws_bytes(R, V))
        _call(x.device, "smx_xent_forward", x.data_ptr(), row_stride, targets.data_ptr(), ignore_index, reduction,
              buf.data_ptr() + 4 * (2 * R + 1), buf.data_ptr(), buf.data_ptr() + 8 * R, *_ws_arg(ws), R, V, _stream(x.device))
        ctx.meta = (row_stride, ignore_index, reduction)
        ctx.save_for_backward(x, targets, buf)
        return buf[2 * R + 1:] if reduction == _lib.SMX_XENT_NONE else buf[2 * R + 1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        x, targets, buf = ctx.saved_tensors
        row_stride, ignore_index, reduction = ctx.meta
        R, V = x.shape
        g = _grad_f32(g)
        grad = torch.empty((R, V), dtype=torch.float32, device=x.device)
        _call(x.device, "smx_xent_backward", g.data_ptr(), x.data_ptr(), row_stride, targets.data_ptr(), ignore_index,
              reduction, buf.data_ptr(), buf.data_ptr() + 8 * R, grad.data_ptr(), R, V, _stream(x.device))
        return grad, None, None, None, None


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100,
                  reduction: str = "mean") -> torch.Tensor:
    """nn.functional.cross_entropy over the LAST dimension: logits (..., V), class-index targets (...); reduction "mean",
    "sum" or "none" (then of the targets' shape, an ignored position at 0).  Native -- each logit read once forward and
    once backward, no host synchronisation, bitwise reproducible -- when the logits are fp32 on a ROCm device, the targets
    int64 on the same device, autocast is off and numel() > 0; F.cross_entropy everywhere else (CPU, bf16 / fp16, under
    torch.autocast, other target dtypes).  A view whose last dimension is contiguous and whose rows share one stride is
    read in place; anything else is made dense first.
    Difference from torch on the native path: a target outside [0, V) that is not `ignore_index` does not raise a
    device-side assert; that row's loss and its gradient row are NaN (the row counts towards the mean)."""
    if reduction not in _XENT_REDUCTION:
        raise ValueError(f"cross_entropy: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    if logits.dim() < 1 or tuple(targets.shape) != tuple(logits.shape[:-1]):
        raise ValueError(f"cross_entropy: logits {tuple(logits.shape)} need targets of shape {tuple(logits.shape[:-1])}, "
                         f"got {tuple(targets.shape)}")
    V = logits.shape[-1]
    native = (logits.is_cuda and logits.dtype == torch.float32 and targets.dtype == torch.int64
              and targets.device == logits.device and logits.numel() > 0 and not torch.is_autocast_enabled())
    if not native:
        out = torch.nn.functional.cross_entropy(logits.reshape(-1, V), targets.reshape(-1), ignore_index=ignore_index,
                                                reduction=reduction)
        return out.view(targets.shape) if reduction == "none" else out
    x, row_stride = _xent_rows(logits)
    out = _CrossEntropy.apply(x, row_stride, targets.reshape(-1).contiguous(), int(ignore_index),
                              _XENT_REDUCTION[reduction])
    return out.view(targets.shape) if reduction == "none" else out


# ---- the byte sampler of generation (csrc/smx_stream.hip, k_sample_bytes) ------------------------------------------------

_SAMPLE_V = 256
_SAMPLE_MAX_RECENT = 65536


def _sample_bytes_torch(l: torch.Tensor, recent: torch.Tensor, u: torch.Tensor, a: dict):
    """The ten steps of smx_sample_bytes (include/smx.h) on (R, 256) fp32 rows as whole-tensor ops on the rows' device:
    what CPU logits and 2-byte logits run.  No host read of a tensor value."""
    dev, ninf = l.device, float("-inf")
    ar = torch.arange(_SAMPLE_V, device=dev)
    r = recent.to(torch.int64)
    ok = (r >= 0) & (r < _SAMPLE_V)
    cnt = torch.zeros(_SAMPLE_V, dtype=torch.int64, device=dev).scatter_add_(0, r.clamp(0, _SAMPLE_V - 1), ok.to(torch.int64))
    seen = (cnt > 0).unsqueeze(0)
    l = torch.where(seen, l / a["rep"], l)
    if a["presence"] != 0.0 or a["frequency"] != 0.0:
        l = torch.where(seen, l - a["presence"] - a["frequency"] * cnt.to(torch.float32), l)
    if a["ascii_only"]:
        l = l.masked_fill(~((ar == 10) | ((ar >= 32) & (ar <= 126))), ninf)
    if a["ban_cr"]:
        l = l.masked_fill(ar == 13, ninf)
    if a["max_run"] > 0 and r.numel() >= a["max_run"]:
        tail = r[r.numel() - a["max_run"]:]
        l = l.masked_fill(((tail == tail[-1]).all() & (ar == tail[-1])).unsqueeze(0), ninf)
    l = l / a["temperature"]
    if a["top_p"] < 1.0:
        sl, si = torch.sort(l, dim=-1, descending=True, stable=True)
        keep = torch.cumsum(torch.softmax(sl, dim=-1), dim=-1) <= a["top_p"]
        keep[:, 0] = True
        kept = ar.unsqueeze(0) < keep.sum(dim=-1, keepdim=True)
        l = torch.full_like(l, ninf).scatter_(1, si, torch.where(kept, sl, torch.full_like(sl, ninf)))
    if a["top_k"] > 0:
        v = torch.topk(l, min(a["top_k"], _SAMPLE_V), dim=-1).values[:, -1:]
        l = torch.where(l < v, torch.full_like(l, ninf), l)
    p = torch.softmax(l, dim=-1)
    live = p > 0
    hit = (torch.cumsum(p, dim=-1) > u.unsqueeze(1)) & live
    first = torch.where(hit, ar, _SAMPLE_V).min(dim=-1).values
    last = torch.where(live, ar, -1).max(dim=-1).values
    return torch.where(first < _SAMPLE_V, first, last).clamp_(0, _SAMPLE_V - 1), p


def sample_bytes(logits: torch.Tensor, recent: Optional[torch.Tensor], u: Optional[torch.Tensor] = None, *,
                 temperature: float = 1.0, top_p: float = 1.0, top_k: int = 0, repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, ascii_only: bool = False,
                 ban_cr: bool = False, max_run_length: int = 0, generator=None, return_probs: bool = False):
    """Draw one byte per row of `logits` (..., 256): ids (...) int64, with return_probs=True (ids, probs (..., 256) fp32).
    The reference's samplers (fft_lm/train_fixed_full.py:651-701, scripts/stream_generate_fast.py:146-170,
    scripts/generate_chunked_overlap_save.py:39-48, 283-292) as one function, in their order: repetition penalty (a plain
    division) and presence / frequency penalties over the bytes of `recent`, the ascii_only / ban_cr bans, the
    max_run_length ban (the last max_run_length ids of `recent` all equal), temperature, nucleus (top_p < 1: the longest
    prefix of the descending softmax whose running sum stays <= top_p, at least one; top_p >= 1: no such step), top-k
    (ties kept), softmax, and the first byte whose running probability exceeds u.
    recent: 1-D uint8 or int64 ids shared by all rows (None or empty: no window), at most 65536, on the logits' device.
    u: uniforms in [0, 1) of shape logits.shape[:-1]; None draws torch.rand on the device from `generator` -- torch's
    generator, which a capturing graph registers, as DropoutState does.
    fp32 logits on a ROCm device run ONE launch (smx_sample_bytes) with no host synchronisation; CPU logits and other
    dtypes run the same definition as whole-tensor torch ops.  The id drawn always has probability > 0.  Not
    differentiable."""
    if not (isinstance(logits, torch.Tensor) and logits.is_floating_point() and logits.dim() >= 1):
        raise TypeError("sample_bytes: logits must be a floating-point tensor (..., 256)")
    if logits.shape[-1] != _SAMPLE_V:
        raise ValueError(f"sample_bytes: the last dimension of logits must be {_SAMPLE_V} (bytes), got {logits.shape[-1]}")
    dev, lead = logits.device, tuple(logits.shape[:-1])
    f32 = lambda v: ctypes.c_float(float(v)).value          # both paths compare and divide by the same fp32 values
    a = {"temperature": f32(temperature), "top_p": f32(top_p), "rep": f32(repetition_penalty),
         "presence": f32(presence_penalty), "frequency": f32(frequency_penalty), "top_k": int(top_k),
         "ascii_only": bool(ascii_only), "ban_cr": bool(ban_cr), "max_run": int(max_run_length)}
    inf = float("inf")
    if not 0.0 < a["temperature"] < inf:
        raise ValueError(f"sample_bytes: temperature must be positive and finite, got {temperature}")
    if not 0.0 < a["rep"] < inf:
        raise ValueError(f"sample_bytes: repetition_penalty must be positive and finite, got {repetition_penalty}")
    if a["top_p"] != a["top_p"] or not (abs(a["presence"]) < inf and abs(a["frequency"]) < inf):
        raise ValueError("sample_bytes: top_p must not be NaN, presence_penalty and frequency_penalty must be finite")
    if a["top_k"] < 0 or a["max_run"] < 0:
        raise ValueError("sample_bytes: top_k and max_run_length must not be negative")
    if recent is None:
        recent = torch.empty(0, dtype=torch.uint8, device=dev)
    if not (isinstance(recent, torch.Tensor) and recent.dtype in (torch.uint8, torch.int64) and recent.dim() == 1):
        raise TypeError("sample_bytes: recent must be a 1-D uint8 or int64 tensor (or None)")
    if recent.device != dev:
        raise ValueError(f"sample_bytes: recent is on {recent.device}, logits on {dev}")
    if recent.numel() > _SAMPLE_MAX_RECENT:
        raise ValueError(f"sample_bytes: recent holds {recent.numel()} ids, at most {_SAMPLE_MAX_RECENT}")
    if u is None:
        u = torch.rand(lead, dtype=torch.float32, device=dev, generator=generator)
    elif not (isinstance(u, torch.Tensor) and tuple(u.shape) == lead and u.device == dev and u.is_floating_point()):
        raise ValueError(f"sample_bytes: u must be a floating-point tensor of shape {lead} on {dev}")
    R = u.numel()
    if not (logits.is_cuda and logits.dtype == torch.float32 and R > 0):
        ids, p = _sample_bytes_torch(logits.detach().reshape(-1, _SAMPLE_V).float(), recent, u.reshape(-1).float(), a)
        return (ids.view(lead), p.view(*lead, _SAMPLE_V)) if return_probs else ids.view(lead)
    x, row_stride = _xent_rows(logits.detach())
    u = u.reshape(-1).to(torch.float32).contiguous()
    if recent.numel() > 1 and recent.stride(0) != 1 or recent.data_ptr() % recent.element_size():
        recent = recent.contiguous()
    ids = torch.empty(R, dtype=torch.int64, device=dev)
    probs = torch.empty((R, _SAMPLE_V), dtype=torch.float32, device=dev) if return_probs else None
    _call(dev, "smx_sample_bytes", x.data_ptr(), row_stride, recent.data_ptr() if recent.numel() else None,
          recent.element_size(), recent.numel(), a["temperature"], a["top_p"], a["top_k"], a["rep"], a["presence"],
          a["frequency"], int(a["ascii_only"]), int(a["ban_cr"]), a["max_run"], u.data_ptr(), ids.data_ptr(), _ptr(probs),
          R, _SAMPLE_V, _stream(dev))
    return (ids.view(lead), probs.view(*lead, _SAMPLE_V)) if return_probs else ids.view(lead)


# ---- byte-spectral feature rows: fft_tensor's byte language model (csrc/smx_byte.hip) ---------------------------------------

@functools.lru_cache(None)
def byte_supported(T: int, k: int, W: int) -> bool:
    """smx_byte_supported: 1 <= T <= 4096, 0 <= k <= min(T / 2, 2048), 1 <= W <= 4096.  (A property of the library.)"""
    return bool(_lib.lib().smx_byte_supported(int(T), int(k), int(W)))


@functools.lru_cache(None)
def _byte_ws_bytes(B: int, P: int, W: int, k: int) -> int:
    return _query("smx_byte_workspace_bytes", B, P, W, k)


class _ByteFeatures(torch.autograd.Function):
    """The (B, P, W) feature rows of byte tokens through smx_byte_features; |S| (B, k) is kept when the band weights
    want a gradient, which smx_byte_grad_bands forms in a fixed order.  The ids carry no gradient."""

    @staticmethod
    def forward(ctx, tokens, bands, k, W, P):
        B, T = tokens.shape
        dev = tokens.device
        out = torch.empty((B, P, W), dtype=torch.float32, device=dev)
        mag = torch.empty((B, k), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] and k > 0 else None
        _call(dev, "smx_byte_features", tokens.data_ptr(), tokens.element_size(), tokens.stride(0), bands.data_ptr(),
              out.data_ptr(), _ptr(mag), B, T, k, W, P, _stream(dev))
        ctx.dims = (B, P, W, k, bands.numel())
        ctx.save_for_backward(mag)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        (mag,) = ctx.saved_tensors
        B, P, W, k, n = ctx.dims
        g = _grad_f32(g)
        gb = torch.empty(n, dtype=torch.float32, device=g.device)
        ws = _workspace(g.device, _byte_ws_bytes(B, P, W, k))
        _call(g.device, "smx_byte_grad_bands", g.data_ptr(), _ptr(mag), gb.data_ptr(), n, *_ws_arg(ws), B, P, W, k,
              _stream(g.device))
        return None, gb, None, None, None


def _byte_features_torch(tokens: torch.Tensor, bands: torch.Tensor, k: int, W: int, P: int) -> torch.Tensor:
    """The same table as whole-tensor ops on the tokens' device (CPU tokens, sizes outside byte_supported): one float64
    FFT of the rows and the shift theorem's rotation by the exact angle 2 pi (f pos mod T) / T -- never the per-position loop.
    Differentiable in `bands` through autograd."""
    B, T = tokens.shape
    dev = tokens.device
    if k == 0:
        return torch.zeros((B, P, W), dtype=torch.float32, device=dev) + bands.sum() * 0
    S = torch.fft.fft(tokens.to(torch.float32).double() / 127.5 - 1.0, dim=1)[:, :k]        # float64: rounded once, below
    mag = S.abs()
    zero = mag == 0
    one = torch.ones((), dtype=S.dtype, device=dev)
    u = torch.where(zero, one, S / torch.where(zero, torch.ones_like(mag), mag))
    f = torch.arange(k, device=dev)
    ang = ((f[None, :] * torch.arange(P, device=dev)[:, None]) % T).double() * (2.0 * torch.pi / T)
    z = u[:, None, :] * torch.complex(torch.cos(ang), torch.sin(ang))[None]
    z = torch.where(zero[:, None, :], one, z).to(torch.complex64)   # angle(0) = 0 at every position
    feat = torch.cat(((mag.float() * bands[:k].to(torch.float32))[:, None, :].expand(B, P, k), z.imag, z.real), dim=-1)
    if 3 * k < W:
        return torch.nn.functional.pad(feat, (0, W - 3 * k))
    return feat[..., :W].contiguous()


def byte_features(tokens: torch.Tensor, bands: torch.Tensor, width: int, positions: bool = True,
                  native: Optional[bool] = None) -> torch.Tensor:
    """The feature rows of fft_tensor's byte models before their projection (reference
    fft_tensor/byte_spectral_model.py:52-97 and fft_tensor/byte_spectral.py:63-98).  tokens (B, T) uint8 or int64 (any
    int64 value, converted as .float() does); s = id / 127.5 - 1, S = fft(s), k = min(width // 2, T // 2).
    positions=True: (B, T, width) fp32, row pos = [|S[:k]| bands[:k], sin, cos of angle(fft(roll(s, -pos))[:k]), zeros]
    cut at `width` columns (ByteSpectralEmbedding); positions=False: (B, width), the row of pos = 0 (ByteSpectralEncoder).
    On a ROCm device with byte_supported(T, k, width) it is ONE launch with no host synchronisation and a fixed-order
    two-launch gradient for `bands`; elsewhere (CPU, T > 4096 ...) the same table as whole-tensor torch ops.  native=False
    takes the torch ops on any device, native=True refuses to.  A bin whose |S| is tiny has phase columns that are
    rounding noise in the reference and here alike.  The ids carry no gradient."""
    if not (isinstance(tokens, torch.Tensor) and tokens.dtype in (torch.uint8, torch.int64) and tokens.dim() == 2):
        raise TypeError("byte_features: tokens must be a (B, T) uint8 or int64 tensor")
    if not (isinstance(bands, torch.Tensor) and bands.is_floating_point() and bands.dim() == 1):
        raise TypeError("byte_features: bands must be a 1-D floating-point tensor")
    W = int(width)
    if W < 1:
        raise ValueError(f"byte_features: width must be positive, got {width}")
    B, T = tokens.shape
    k = min(W // 2, T // 2)
    if bands.numel() < k:
        raise ValueError(f"byte_features: bands holds {bands.numel()} weights, {k} bins are kept")
    if bands.device != tokens.device:
        raise ValueError(f"byte_features: bands is on {bands.device}, tokens on {tokens.device}")
    P = T if positions else 1
    if B == 0 or T == 0:
        out = torch.zeros((B, P, W), dtype=torch.float32, device=tokens.device)
    else:
        can = tokens.is_cuda and bands.dtype == torch.float32 and bands.numel() > 0 and byte_supported(T, k, W)
        if native and not can:
            raise ValueError(f"byte_features: no native launch for T={T}, k={k}, width={W} on {tokens.device}")
        if can and native is not False:
            tokens = _token_rows(tokens)
            out = _ByteFeatures.apply(tokens, _dense(bands), k, W, P)
        else:
            out = _byte_features_torch(tokens, bands, k, W, P)
    return out if positions else out[:, 0, :]


# ---- multi-pattern exact byte search: the corpus scan of the parroting score (csrc/smx_match.hip) ---------------------------

@functools.lru_cache(None)
def match_supported(S: int, L: int) -> bool:
    """smx_match_supported: 1 <= S <= 256, 4 <= L <= 256, S * L <= 32768.  (A property of the library.)"""
    return bool(_lib.lib().smx_match_supported(int(S), int(L)))


@functools.lru_cache(None)
def _match_ws_bytes(S: int, L: int) -> int:
    return _query("smx_match_workspace_bytes", S, L)


def _find_snippets_host(corpus: bytes, snips: bytes, S: int, L: int) -> list:
    """the definition: bytes.find per snippet"""
    return [corpus.find(snips[s * L:(s + 1) * L]) for s in range(S)]


def _host_bytes(t) -> bytes:
    return t if isinstance(t, bytes) else t.detach().contiguous().cpu().numpy().tobytes()


def find_snippets(corpus_u8, snips_u8: torch.Tensor, *, max_workgroups: int = 0) -> torch.Tensor:
    """first (S,) int64 on the snippets' device: first[s] = the smallest p with corpus[p : p + L] == snips[s], -1 when the
    snippet does not occur -- `bytes.find` for S snippets of L bytes at once, the scan of the reference's parroting_score
    (fft_lm/train_fixed_full.py:200-204, one host pass over the corpus per absent snippet).
    corpus_u8: a 1-D uint8 tensor or `bytes`; snips_u8: (S, L) uint8.  A corpus on a ROCm device with
    match_supported(S, L) is ONE pass over the corpus (smx_match_first: no host synchronisation, nothing allocated beside
    the answer, capturable, bitwise reproducible; a view at any byte offset is read in place, a strided one is made
    contiguous).  A CPU or `bytes` corpus, and any other (S, L), compute the same definition with bytes.find on the
    host.  max_workgroups (> 0) caps the native scan's workgroups: a test and tuning knob."""
    if not (isinstance(snips_u8, torch.Tensor) and snips_u8.dtype == torch.uint8 and snips_u8.dim() == 2):
        raise TypeError("find_snippets: snips_u8 must be an (S, L) uint8 tensor")
    if not isinstance(corpus_u8, bytes) and not (isinstance(corpus_u8, torch.Tensor) and corpus_u8.dtype == torch.uint8
                                                  and corpus_u8.dim() == 1):
        raise TypeError("find_snippets: corpus_u8 must be a 1-D uint8 tensor or bytes")
    S, L = snips_u8.shape
    if L < 1:
        raise ValueError("find_snippets: snippets must hold at least one byte")
    if max_workgroups < 0:
        raise ValueError(f"find_snippets: max_workgroups must not be negative, got {max_workgroups}")
    if S == 0:
        return torch.empty(0, dtype=torch.int64, device=snips_u8.device)
    if isinstance(corpus_u8, bytes) or not corpus_u8.is_cuda or not match_supported(S, L):
        first = _find_snippets_host(_host_bytes(corpus_u8), _host_bytes(snips_u8), S, L)
        return torch.tensor(first, dtype=torch.int64, device=snips_u8.device)
    dev = corpus_u8.device
    _require("corpus_u8", corpus_u8, (torch.uint8,), _ANY_PATH, what="a 1-D uint8 tensor", dim=1)
    if snips_u8.device != dev:
        raise ValueError(f"find_snippets: snips_u8 is on {snips_u8.device}, corpus_u8 on {dev}")
    _require("snips_u8", snips_u8, (torch.uint8,), _ANY_PATH, what="an (S, L) uint8 tensor", dim=2)
    corpus, snips = corpus_u8.contiguous(), snips_u8.contiguous()
    first = torch.empty(S, dtype=torch.int64, device=dev)
    ws = _workspace(dev, _match_ws_bytes(S, L))
    _call(dev, "smx_match_first", corpus.data_ptr() if corpus.numel() else None, corpus.numel(), snips.data_ptr(), S, L,
          first.data_ptr(), *_ws_arg(ws), int(max_workgroups), _stream(dev))
    return first


# ---- sparse spectral tensor: top-k sparsify, scatter and the N-D transform (csrc/smx_sst.hip) -----------------------------------

@functools.lru_cache(None)
def topk_supported(n: int) -> bool:
    """smx_topk_supported: 1 <= n < 2**31.  (A property of the library.)"""
    return bool(_lib.lib().smx_topk_supported(int(n)))


@functools.lru_cache(512)
def _topk_ws_bytes(n: int) -> int:
    return _query("smx_topk_workspace_bytes", n)


def _squared_keys(flat: torch.Tensor) -> torch.Tensor:
    """key = bits(fl(fl(re re) + fl(im im))) & 0x7fffffff as int32 (never negative, so signed order = unsigned order):
    three whole-tensor fp32 ops, each rounded once, no FMA."""
    ri = torch.view_as_real(flat)
    re, im = ri[..., 0], ri[..., 1]
    return (re * re + im * im).view(torch.int32) & 0x7fffffff


def _sparsify_torch(flat: torch.Tensor, k: int):
    """the definition of sparsify_topk with whole-tensor torch ops"""
    keys = _squared_keys(flat.detach())
    t = torch.kthvalue(keys, keys.numel() - k + 1).values           # the k-th largest key
    idx = torch.nonzero(keys >= t).flatten()
    return flat[idx], idx


def sparsify_topk(freq: torch.Tensor, sparsity: Optional[float] = None, *, k: Optional[int] = None,
                  max_workgroups: int = 0):
    """(coeffs (m,) complex64, flat_indices (m,) int64): the elements of the flattened complex64 `freq` whose squared
    magnitude is at least the k-th largest one, in ascending index order -- the reference's _sparsify_pytorch
    (fft_tensor/tensor.py:136-144: abs, topk, >=, nonzero, masked gather) without the sort and the four extra passes.
    k = max(1, int(numel * sparsity)), the reference's expression, or `k` itself.  Ties at the threshold are all kept
    (m >= k), as the reference's `magnitude >= threshold` keeps them; the order is that of the key
    bits(fl(fl(re re) + fl(im im))) & 0x7fffffff in fp32, so a NaN ranks above inf, and two magnitudes that torch.abs
    tells apart in the last bit may tie or swap here.
    On a ROCm device: smx_topk_select (an exact radix select, three passes over the spectrum, plus one that counts), ONE
    host read of m (the reference's nonzero synchronises too), smx_topk_compact into exactly sized outputs; bitwise
    reproducible.  CPU tensors, numel >= 2**31 and inputs that require grad compute the same definition with
    whole-tensor torch ops.  Not differentiable (as in the reference): the native path builds no graph; on the torch path
    the gather carries a gradient as any indexing does.  max_workgroups (> 0) caps the native tile walks: a test and
    tuning knob."""
    if not (isinstance(freq, torch.Tensor) and freq.dtype == torch.complex64):
        raise TypeError("sparsify_topk: freq must be a complex64 tensor")
    n = freq.numel()
    if n == 0:
        raise ValueError("sparsify_topk: freq is empty")
    if (sparsity is None) == (k is None):
        raise ValueError("sparsify_topk: give exactly one of sparsity and k")
    k = max(1, int(n * sparsity)) if k is None else int(k)
    if k < 1 or k > n:
        raise ValueError(f"sparsify_topk: k must be in 1..numel, got k={k} numel={n}")
    if max_workgroups < 0:
        raise ValueError(f"sparsify_topk: max_workgroups must not be negative, got {max_workgroups}")
    flat = freq.resolve_conj().contiguous().view(-1)             # complex64 storage is 8-byte aligned at any offset
    if not flat.is_cuda or flat.requires_grad or not topk_supported(n):
        return _sparsify_torch(flat, k)
    dev = flat.device
    result = torch.empty(2, dtype=torch.int64, device=dev)          # m, threshold key
    ws = _workspace(dev, _topk_ws_bytes(n))
    _call(dev, "smx_topk_select", flat.data_ptr(), n, k, result.data_ptr(), *_ws_arg(ws), int(max_workgroups), _stream(dev))
    m = int(result[0].item())
    coeffs = torch.empty(m, dtype=torch.complex64, device=dev)
    idx = torch.empty(m, dtype=torch.int64, device=dev)
    _call(dev, "smx_topk_compact", flat.data_ptr(), n, result.data_ptr(), coeffs.data_ptr(), idx.data_ptr(), m,
          *_ws_arg(ws), int(max_workgroups), _stream(dev))       # the workspace is as smx_topk_select left it
    return coeffs, idx


def sparse_scatter(coeffs: torch.Tensor, flat_indices: torch.Tensor, shape, *, assume_ascending: bool = False,
                   max_workgroups: int = 0) -> torch.Tensor:
    """A complex64 tensor of `shape`: zeros with flat[flat_indices[j]] = coeffs[j] -- the reference's _scatter_pytorch
    (fft_tensor/tensor.py:194-203).  On a ROCm device with assume_ascending=True (the caller's promise that
    flat_indices is strictly ascending and inside [0, numel): what sparsify_topk returns) it is ONE native launch that
    writes the output exactly once (smx_sparse_scatter; a broken promise gives unspecified contents, nothing else).
    Otherwise zeros + index_put_.  Not differentiable on the native path (coeffs that require grad take the torch ops)."""
    if not (isinstance(coeffs, torch.Tensor) and coeffs.dtype == torch.complex64 and coeffs.dim() == 1):
        raise TypeError("sparse_scatter: coeffs must be a 1-D complex64 tensor")
    if not (isinstance(flat_indices, torch.Tensor) and flat_indices.dtype == torch.int64
            and flat_indices.shape == coeffs.shape):
        raise TypeError("sparse_scatter: flat_indices must be an int64 tensor of coeffs' length")
    if flat_indices.device != coeffs.device:
        raise ValueError(f"sparse_scatter: flat_indices is on {flat_indices.device}, coeffs on {coeffs.device}")
    if max_workgroups < 0:
        raise ValueError(f"sparse_scatter: max_workgroups must not be negative, got {max_workgroups}")
    shape = tuple(int(s) for s in shape)
    n, m = math.prod(shape), coeffs.numel()
    if coeffs.is_cuda and assume_ascending and not coeffs.requires_grad and m <= n and n > 0 and topk_supported(n):
        dev = coeffs.device
        out = torch.empty(shape, dtype=torch.complex64, device=dev)
        c, i = coeffs.resolve_conj().contiguous(), flat_indices.contiguous()
        _call(dev, "smx_sparse_scatter", c.data_ptr() if m else None, i.data_ptr() if m else None, m, out.data_ptr(), n,
              int(max_workgroups), _stream(dev))
        return out
    out = torch.zeros(n, dtype=torch.complex64, device=coeffs.device)
    out.index_put_((flat_indices,), coeffs)
    return out.reshape(shape)


def _walk_axes(z: torch.Tensor, fft1d, naxes: int) -> torch.Tensor:
    """1-D transforms along the first `naxes` axes of the contiguous `z`, each as the middle axis of a (B, N, D) view"""
    shape = tuple(z.shape)
    out = z
    for i, n in enumerate(shape[:naxes]):
        if n > 1:
            out = fft1d(out.reshape(math.prod(shape[:i]), n, math.prod(shape[i + 1:]))).contiguous()
    return out.reshape(shape)


def _axis_walk(z: torch.Tensor, fft1d) -> torch.Tensor:
    """The N-D DFT of `z` as 1-D transforms along each axis in turn.  Axis i of a contiguous tensor is the middle axis
    of the view (prod(shape[:i]), shape[i], prod(shape[i+1:])), so nothing is transposed; `fft1d` maps a contiguous
    (B, N, D) complex tensor to its DFT along dim 1.  Axes of length 1 are skipped."""
    out = _walk_axes(z.contiguous(), fft1d, z.dim())
    if out.data_ptr() == z.data_ptr():                   # no axis longer than 1: the transform is the identity
        out = out.clone()
    return out


def _check_c64(name: str, z) -> None:
    if not (isinstance(z, torch.Tensor) and z.dtype == torch.complex64):
        raise TypeError(f"{name}: z must be a complex64 tensor")


# ---- the DFT along the contiguous last axis (csrc/smx_rowfft.hip) and the N-D transforms on it -----------------------------------

ROWFFT_MAX_N = _lib.SMX_ROWFFT_MAX_N


@functools.lru_cache(None)
def rowfft_supported(n: int) -> bool:
    """True where smx_rowfft transforms rows of n points: n a power of two from 2 to 4096"""
    return bool(_lib.lib().smx_rowfft_supported(int(n)))


def row_fft_raw(x: torch.Tensor, *, conj_in: bool = False, conj_out: bool = False, real_out: bool = False,
                scale: float = 1.0, out: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> torch.Tensor:
    """One launch of smx_rowfft over the last axis of `x` (any tensor with at least one dimension, on a ROCm device):
        out[..., k] = scale * sum_j a[..., j] exp(-2 pi i j k / n),   a = x, or conj(x) with conj_in,
    conjugated with conj_out, its real part alone (float32) with real_out.  complex64 input gives the complex transform;
    float32 input is taken as (x, 0) without a complex copy of it (SMX_ROWFFT_REAL_IN).  `out`: a dense 16-byte aligned
    tensor of x's shape and the result's dtype to write into; it may be `x` itself when both have the same dtype.
    n must satisfy rowfft_supported (SmxError otherwise).  Not differentiable: row_fft / row_ifft are."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dtype not in (torch.complex64, torch.float32):
        raise TypeError(f"x must be complex64 or float32, got {x.dtype}")
    if x.dim() < 1:
        raise ValueError("row_fft_raw: x must have at least one dimension")
    mwg = _check_wg("row_fft_raw", max_workgroups)
    _require("x", x, None, _ANY_PATH)
    dev, n = x.device, int(x.shape[-1])
    xd = _dense(x)
    odt = torch.float32 if real_out else torch.complex64
    if out is None:
        out = torch.empty(x.shape, dtype=odt, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == odt and out.shape == x.shape
              and out.is_contiguous() and out.data_ptr() % 16 == 0 and not (out.is_complex() and out.is_conj())):
        raise ValueError(f"row_fft_raw: out must be a dense, 16-byte aligned {odt} tensor of shape {tuple(x.shape)} on {dev}")
    flags = (_lib.SMX_ROWFFT_CONJ_IN if conj_in else 0) | (_lib.SMX_ROWFFT_CONJ_OUT if conj_out else 0) \
        | (_lib.SMX_ROWFFT_REAL_IN if x.dtype == torch.float32 else 0) | (_lib.SMX_ROWFFT_REAL_OUT if real_out else 0)
    rows = xd.numel() // n if n else 0
    _call(dev, "smx_rowfft", xd.data_ptr(), out.data_ptr(), rows, n, flags, float(scale), mwg, _stream(dev))
    return out


class _RowFFT(torch.autograd.Function):
    """Y = scale * F a along the last axis, a = z or conj(z), conjugated on the way out or not: fft (inverse False:
    flags 0, scale 1) and ifft (inverse True: both conjugations, scale 1 / n, as ifft z = conj(F conj z) / n).
    Backward, in torch's convention grad_z = A^H grad_Y for Y = A z: F is symmetric, so for fft A^H = conj(F) and
    grad_z = conj(F conj(g)) -- both conjugations, scale 1; for ifft A = conj(F) / n, A^H = F / n and grad_z = F g / n --
    no flag, scale 1 / n.  Either is one launch of the same kernel."""

    @staticmethod
    def forward(ctx, z, inverse):
        ctx.inverse = inverse
        return row_fft_raw(z, conj_in=inverse, conj_out=inverse, scale=1.0 / z.shape[-1] if inverse else 1.0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        inv = ctx.inverse
        return row_fft_raw(_grad_c64(g), conj_in=not inv, conj_out=not inv, scale=1.0 / g.shape[-1] if inv else 1.0), None


def _row_native(t: torch.Tensor) -> bool:
    """the last axis of `t` has a native transform: a ROCm tensor with at least one axis whose last length is supported"""
    return t.is_cuda and t.dim() >= 1 and rowfft_supported(t.shape[-1])


def _seq_rows(z: torch.Tensor) -> torch.Tensor:
    """the composition the last axis ran as before smx_rowfft, and still does for other lengths: a one-channel batch"""
    return seq_fft(z.reshape(-1, z.shape[-1], 1)).reshape(z.shape)


def row_fft(z: torch.Tensor) -> torch.Tensor:
    """torch.fft.fft(z, dim=-1) of a complex64 tensor, differentiable.  On a ROCm device with rowfft_supported(n): one
    launch of smx_rowfft per direction; other lengths there: seq_fft on the one-channel view; CPU tensors: torch.fft."""
    _check_c64("row_fft", z)
    if not z.is_cuda or z.dim() < 1 or z.numel() == 0:
        return torch.fft.fft(z, dim=-1)
    if not rowfft_supported(z.shape[-1]):
        return _seq_rows(z)
    return _RowFFT.apply(z, False)


def row_ifft(z: torch.Tensor) -> torch.Tensor:
    """torch.fft.ifft(z, dim=-1) of a complex64 tensor, differentiable: see row_fft"""
    _check_c64("row_ifft", z)
    if not z.is_cuda or z.dim() < 1 or z.numel() == 0:
        return torch.fft.ifft(z, dim=-1)
    if not rowfft_supported(z.shape[-1]):
        return _seq_rows(z.conj()).conj() / z.shape[-1]
    return _RowFFT.apply(z, True)


def fftn(z: torch.Tensor) -> torch.Tensor:
    """torch.fft.fftn(z) of a complex64 tensor over all its axes.  On a ROCm device the last axis is one launch of the
    native row transform (row_fft_raw) where rowfft_supported(its length), and the other axes -- and the last one at
    other lengths -- are the native sequence transform (seq_fft) axis by axis on views of the contiguous tensor: no FFT
    library runs, nothing is transposed.  CPU tensors (and empty ones, and inputs that require grad) use torch.fft.
    Not differentiable on the device path."""
    _check_c64("fftn", z)
    if not z.is_cuda or z.numel() == 0 or z.requires_grad:
        return torch.fft.fftn(z)
    if _row_native(z):
        return _walk_axes(row_fft_raw(z), seq_fft_raw, z.dim() - 1)
    return _axis_walk(z.resolve_conj(), seq_fft_raw)


def _ifftn_device(z: torch.Tensor, real_out: bool) -> torch.Tensor:
    """conj(fftn(conj z)) / numel with the last axis last: its launch conjugates and scales on the way out (and keeps the
    real part alone with real_out); a tensor whose other axes all have length 1 is conjugated on the way in as well"""
    if z.dim() == 1 or math.prod(z.shape[:-1]) == 1:
        return row_fft_raw(z, conj_in=True, conj_out=True, real_out=real_out, scale=1.0 / z.numel())
    lead = _walk_axes(z.conj().resolve_conj().contiguous(), seq_fft_raw, z.dim() - 1)
    return row_fft_raw(lead, conj_out=True, real_out=real_out, scale=1.0 / z.numel())


def ifftn(z: torch.Tensor) -> torch.Tensor:
    """torch.fft.ifftn(z) of a complex64 tensor over all its axes: conj(fftn(conj z)) / numel on a ROCm device (see
    fftn; with a native last axis the closing conjugation and division are part of its launch), torch.fft elsewhere.
    Not differentiable on the device path."""
    _check_c64("ifftn", z)
    if not z.is_cuda or z.numel() == 0 or z.requires_grad:
        return torch.fft.ifftn(z)
    if _row_native(z):
        return _ifftn_device(z, False)
    out = _axis_walk(z.conj().resolve_conj(), seq_fft_raw)
    return torch.conj_physical(out).div_(z.numel())


def fftn_real(x: torch.Tensor) -> torch.Tensor:
    """fftn(x.to(complex64)) of a real tensor.  float32 on a ROCm device with a native last axis: that axis runs first and
    reads the fp32 rows as they are (SMX_ROWFFT_REAL_IN; the axis order of a separable transform is free), so no complex
    copy of the input is made.  Everything else: fftn of the complex copy."""
    if not (isinstance(x, torch.Tensor) and x.is_floating_point()):
        raise TypeError("fftn_real: x must be a real floating-point tensor")
    if x.dtype == torch.float32 and x.numel() > 0 and not x.requires_grad and _row_native(x):
        return _walk_axes(row_fft_raw(x), seq_fft_raw, x.dim() - 1)
    return fftn(x.to(torch.complex64))


def ifftn_real(z: torch.Tensor) -> torch.Tensor:
    """ifftn(z).real as a dense float32 tensor.  On a ROCm device with a native last axis that axis runs last and writes
    the real part alone (SMX_ROWFFT_REAL_OUT): the complex result is never stored."""
    _check_c64("ifftn_real", z)
    if z.is_cuda and z.numel() > 0 and not z.requires_grad and _row_native(z):
        return _ifftn_device(z, True)
    return ifftn(z).real


# ---- the frequency-domain transformer ops: attention and layernorm (csrc/smx_freq.hip) --------------------------------------

_fattn_ws_cache = _Memo()
FREQ_LN_MAX_D = _lib.SMX_FREQ_LN_MAX_D


def _freq_native(*ts) -> bool:
    """complex64 tensors on one ROCm device that autograd does not follow: what the forward-only kernels take"""
    t0 = ts[0]
    if not all(isinstance(t, torch.Tensor) and t.dtype == torch.complex64 and t.is_cuda and t.device == t0.device
               for t in ts):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in ts))


def _f32_finite_nonzero(v) -> bool:
    """a Python number that is finite and not 0 once it is the C entry's float argument (1e-50 is 0 there, 1e39 inf)"""
    try:
        f = ctypes.c_float(v).value
    except (OverflowError, TypeError):
        return False
    return math.isfinite(f) and f != 0.0


def _frequency_attention_torch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, temperature) -> torch.Tensor:
    """the reference's op sequence (fft_tensor/frequency_ops.py:166-185) as whole-tensor torch ops"""
    scores = (torch.abs(q * torch.conj(k)) / temperature).mean(dim=-1)
    return torch.softmax(scores, dim=-1).unsqueeze(-1) * v


def _complex_rows(t: torch.Tensor) -> torch.Tensor:
    """`t` with a contiguous innermost axis (any strides on the others): itself where it has one, a dense copy otherwise"""
    t = t.resolve_conj()
    return t if t.shape[-1] <= 1 or t.stride(-1) == 1 else t.contiguous()


def frequency_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, temperature: float = 1.0, *,
                        merge_heads: bool = False) -> torch.Tensor:
    """The reference's FrequencyAttention.frequency_attention for complex q, k, v of shape (B, H, N, D):
        s[b, h, n] = mean_d(|q conj(k)| / temperature),  p = softmax_n(s),  out = p[..., None] v      (B, H, N, D).
    merge_heads=True returns the same values as `out.transpose(1, 2).contiguous().view(B, N, H * D)`, what a multi-head
    layer does next.
    Native (smx_freq_attention_forward: one launch that reads q and k once and writes a score per row, one that takes the
    softmax statistics and scales v; 32 bytes of traffic per element, bitwise reproducible) for complex64 tensors of one
    shape on a ROCm device with a float temperature that is finite and not 0 in fp32, B H N < 2**31 and N <= 2**30, when no
    operand requires grad or grad mode is off.
    The operands are read through their strides -- head-transposed views of (B, N, H, D) tensors cost no copy; only an
    operand whose innermost stride is not 1 is copied -- and with merge_heads the result is written in (B, N, H D)
    layout directly.  Everything else (CPU tensors, other dtypes, broadcasting shapes, operands that require grad) runs
    the definition as the reference's whole-tensor torch ops, so it differentiates and fails exactly as the reference
    does.  There is no native backward."""
    native = (isinstance(temperature, (int, float)) and _f32_finite_nonzero(temperature)
              and isinstance(q, torch.Tensor) and q.dim() == 4 and _freq_native(q, k, v)
              and q.shape == k.shape == v.shape
              and q.shape[0] * q.shape[1] * q.shape[2] < 2 ** 31 and q.shape[2] <= 2 ** 30)      # the entry's limits
    if not native:
        out = _frequency_attention_torch(q, k, v, temperature)
        if merge_heads:
            B, H, N, D = out.shape
            out = out.transpose(1, 2).contiguous().view(B, N, H * D)
        return out
    B, H, N, D = q.shape
    dev = q.device
    store = torch.empty((B, N, H, D) if merge_heads else (B, H, N, D), dtype=torch.complex64, device=dev)
    out = store.permute(0, 2, 1, 3) if merge_heads else store
    if store.numel():
        q, k, v = _complex_rows(q), _complex_rows(k), _complex_rows(v)
        ws = _workspace(dev, _fattn_ws_cache.get((B, H, N), lambda: _query("smx_freq_attention_workspace_bytes", B, H, N)))
        _call(dev, "smx_freq_attention_forward", q.data_ptr(), *q.stride()[:3], k.data_ptr(), *k.stride()[:3],
              v.data_ptr(), *v.stride()[:3], out.data_ptr(), *out.stride()[:3], float(temperature), *_ws_arg(ws),
              B, H, N, D, _stream(dev))
    return store.view(B, N, H * D) if merge_heads else store


def _frequency_layernorm_torch(z: torch.Tensor, eps: float) -> torch.Tensor:
    """the reference's op sequence (fft_tensor/frequency_ops.py:390-401)"""
    magnitude = torch.abs(z)
    mean_mag = magnitude.mean(dim=-1, keepdim=True)
    std_mag = magnitude.std(dim=-1, keepdim=True)
    return (magnitude - mean_mag) / (std_mag + eps) * torch.exp(1j * torch.angle(z))


def frequency_layernorm(z: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """The reference's frequency_layernorm over the last axis of a complex tensor: with m = |z|,
        out = (m - mean(m)) / (std(m) + eps) * exp(i angle(z)),
    std unbiased as torch.std's default (a last axis of 1 gives NaN, as in the reference) and exp(i angle(0)) = 1.
    Native (smx_freq_layernorm_forward: one launch, one wavefront per row with the row in registers, 16 bytes of traffic
    per element, bitwise reproducible; the unit phase is z / |z|, no trigonometry) for a complex64 tensor on a ROCm device
    whose last axis is at most FREQ_LN_MAX_D = 1024 wide, when it does not require grad or grad mode is off.  Wider rows,
    CPU tensors, other dtypes and inputs that require grad run the reference's whole-tensor torch ops, so they
    differentiate exactly as the reference does.  There is no native backward."""
    native = (isinstance(z, torch.Tensor) and z.dim() >= 1 and _freq_native(z) and z.numel() > 0
              and z.shape[-1] <= FREQ_LN_MAX_D and isinstance(eps, (int, float)))
    if not native:
        return _frequency_layernorm_torch(z, eps)
    zd = _dense(z)
    out = torch.empty_like(zd)
    D = z.shape[-1]
    _call(z.device, "smx_freq_layernorm_forward", zd.data_ptr(), out.data_ptr(), float(eps), zd.numel() // D, D,
          _stream(z.device))
    return out


# ---- the per-bin channel contraction of the FFT convolutions (csrc/smx_fconv.hip) --------------------------------------------

@functools.lru_cache(4096)
def bin_contract_supported(B: int, P: int, Ci: int, Co: int) -> bool:
    """smx_bin_contract_supported: every size at least 1, P < 2**31, every operand below 2**40 elements.  (A property of the
    library.)"""
    if not all(0 < v < 2 ** 31 for v in (B, Ci, Co)) or not 0 < P < 2 ** 62:
        return False
    return bool(_lib.lib().smx_bin_contract_supported(int(B), int(P), int(Ci), int(Co)))


class _BinContract(torch.autograd.Function):
    """y[b, p, o] = sum_i x[b, p, i] w[p, i, o] (smx_bin_contract_forward) with its native backward
    (smx_bin_contract_backward; torch's convention, grad = dL/dRe + i dL/dIm):
        gx[b, p, i] = sum_o gy[b, p, o] conj(w[p, i, o]),   gw[p, i, o] = sum_b conj(x[b, p, i]) gy[b, p, o].
    Only the gradients autograd asks for are computed (a launch each)."""

    @staticmethod
    def forward(ctx, x, w, max_workgroups):
        ctx.smx_opts = _lib.effective_options()
        B, P, Ci = x.shape
        Co = w.shape[2]
        y = torch.empty((B, P, Co), dtype=torch.complex64, device=x.device)
        _call(x.device, "smx_bin_contract_forward", x.data_ptr(), w.data_ptr(), y.data_ptr(), B, P, Ci, Co, max_workgroups,
              _stream(x.device))
        ctx.save_for_backward(x, w)
        ctx.mwg = max_workgroups
        return y

    @staticmethod
    @once_differentiable
    @_under_forward_options
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        B, P, Ci = x.shape
        Co = w.shape[2]
        gy = _grad_c64(gy)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        if gx is not None or gw is not None:
            _call(x.device, "smx_bin_contract_backward", x.data_ptr(), w.data_ptr(), gy.data_ptr(), _ptr(gx), _ptr(gw), B, P,
                  Ci, Co, ctx.mwg, _stream(x.device))
        return gx, gw, None


def bin_contract(x: torch.Tensor, w: torch.Tensor, *, max_workgroups: int = 0) -> torch.Tensor:
    """torch.einsum("bpi,pio->bpo", x, w): one small complex matrix product per bin p, channels innermost on every operand
    -- x (B, P, Ci), w (P, Ci, Co), the result (B, P, Co) -- which is the layout rfft / seq_fft produce, so nothing is
    transposed between the transforms and the contraction.  It is what the reference's FFT convolutions compute as
    `(x_freq.unsqueeze(1) * w_freq.unsqueeze(0)).sum(dim=2)` (fft_tensor/optimized_ops.py:183-187, :247-251) over a
    materialised (B, Co, Ci, bins) product.
    Native (smx_bin_contract_forward / _backward: fp32 FMAs, every sum in ascending index order, bitwise reproducible,
    capturable) for complex64 operands on one ROCm device with sizes inside smx_bin_contract_supported, whether or not
    they require grad: this op has a native backward (gx and gw, a launch each, only those asked for).  Everything else
    (CPU tensors, other dtypes, empty operands, sizes beyond the limits) runs the einsum.  max_workgroups (> 0) caps the
    native tile walks: a test and tuning knob."""
    if not (isinstance(x, torch.Tensor) and isinstance(w, torch.Tensor) and x.dim() == 3 and w.dim() == 3):
        raise TypeError("bin_contract: x must be a (B, P, Ci) tensor and w a (P, Ci, Co) tensor")
    if x.shape[1:] != w.shape[:2]:
        raise ValueError(f"bin_contract: x is {tuple(x.shape)}, w is {tuple(w.shape)}: need (B, P, Ci) and (P, Ci, Co)")
    if max_workgroups < 0:
        raise ValueError(f"bin_contract: max_workgroups must not be negative, got {max_workgroups}")
    native = (x.dtype == torch.complex64 and w.dtype == torch.complex64 and x.is_cuda and w.device == x.device
              and bin_contract_supported(x.shape[0], x.shape[1], x.shape[2], w.shape[2]))
    if not native:
        return torch.einsum("bpi,pio->bpo", x, w)
    return _BinContract.apply(_dense(x), _dense(w), int(max_workgroups))


# ---- the polar and log8 codecs of the compressed spectra (csrc/smx_quant.hip) ---------------------------------------------------

def _codec_native(*ts, bits=()) -> bool:
    """tensors on one ROCm device that autograd does not follow, bit counts the one-byte planes hold"""
    t0 = ts[0]
    if not (t0.is_cuda and all(t.device == t0.device for t in ts) and all(1 <= int(b) <= 8 for b in bits)):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in ts))


def _flat(t: torch.Tensor) -> torch.Tensor:
    """Contiguous, in place where it already is: the codecs take a complex64 tensor at any 8-byte address, an fp32 one at
    any 4-byte address and a byte plane at any address, so a view such as z[1:] or mag_q[3:] is not copied (_dense would)."""
    if t.is_complex():
        t = t.resolve_conj()
    return t.contiguous()


def _check_wg(name: str, max_workgroups: int) -> int:
    if max_workgroups < 0:
        raise ValueError(f"{name}: max_workgroups must not be negative, got {max_workgroups}")
    return int(max_workgroups)


def _check_planes(name: str, a: torch.Tensor, b: torch.Tensor) -> None:
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
        raise TypeError(f"{name}: the code planes must be tensors")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"{name}: the code planes differ: {tuple(a.shape)} on {a.device}, {tuple(b.shape)} on {b.device}")


@functools.lru_cache(64)
def _polar_range_ws_bytes(n: int) -> int:
    return _query("smx_polar_range_workspace_bytes", n)


def polar_range(z: torch.Tensor, *, max_workgroups: int = 0) -> torch.Tensor:
    """(2,) float32 on z's device: the minimum and maximum over the elements of log2(max(|z|, 1e-9)), the adaptive range
    of the reference's PolarQuantizer.quantize (fft_tensor/polar_quantization.py:29-32: abs, clamp, log2, min, max and two
    host reads).  No host read happens here; the caller makes one (`.tolist()`).
    complex64 on a ROCm device: smx_polar_range, two launches over re^2 + im^2 (log2 is monotone, so it is applied to the
    two ends only); a NaN element does not enter.  Everything else runs the reference's ops.  Not differentiable."""
    if not isinstance(z, torch.Tensor):
        raise TypeError("polar_range: z must be a tensor")
    if z.numel() == 0:
        raise ValueError("polar_range: z is empty")
    mwg = _check_wg("polar_range", max_workgroups)
    if not (z.dtype == torch.complex64 and _codec_native(z)):
        log_mag = torch.log2(torch.abs(z).clamp(min=1e-9))
        return torch.stack((log_mag.min(), log_mag.max())).detach()
    dev, zc = z.device, _flat(z)
    out2 = torch.empty(2, dtype=torch.float32, device=dev)
    ws = _workspace(dev, _polar_range_ws_bytes(zc.numel()))
    _call(dev, "smx_polar_range", zc.data_ptr(), zc.numel(), out2.data_ptr(), *_ws_arg(ws), mwg, _stream(dev))
    return out2


def polar_quantize(z: torch.Tensor, mag_bits: int, phase_bits: int, mag_range, *, max_workgroups: int = 0):
    """(mag_q, phase_q), two uint8 tensors of z's shape: PolarQuantizer.quantize for a given range (mag_min, mag_max) of
    Python floats (fft_tensor/polar_quantization.py:25-42).  With Lm = 2**mag_bits - 1 and Lp = 2**phase_bits - 1:
        mag_q   = clamp(round((log2(max(|z|, 1e-9)) - mag_min) / (mag_max - mag_min + 1e-9) * Lm), 0, Lm)
        phase_q = clamp(round((angle(z) + pi) / (2 pi) * Lp), 0, Lp)            (round: half to even)
    complex64 on a ROCm device with both bit counts in 1..8: smx_polar_quantize, ONE launch that reads 8 bytes and writes 2
    per element (the reference: about fifteen whole-tensor passes); a code can differ from the reference's by one where
    the value before rounding lies within about 1e-5 of a rounding boundary (the device's log2 and atan2 differ from the
    host's in the last bits).  Everything else -- CPU tensors, other dtypes, inputs that require grad, bit counts above 8,
    whose codes wrap in the uint8 cast exactly as the reference's do -- runs the reference's op sequence.  Not
    differentiable."""
    if not isinstance(z, torch.Tensor):
        raise TypeError("polar_quantize: z must be a tensor")
    mag_min, mag_max = (float(v) for v in mag_range)
    mwg = _check_wg("polar_quantize", max_workgroups)
    mag_levels, phase_levels = 2 ** mag_bits, 2 ** phase_bits
    if not (z.dtype == torch.complex64 and z.numel() > 0 and _codec_native(z, bits=(mag_bits, phase_bits))):
        mag = torch.abs(z)
        phase = torch.angle(z)
        log_mag = torch.log2(mag.clamp(min=1e-9))
        mag_norm = (log_mag - mag_min) / (mag_max - mag_min + 1e-9)
        mag_q = (mag_norm * (mag_levels - 1)).round().clamp(0, mag_levels - 1).to(torch.uint8)
        phase_norm = (phase + math.pi) / (2 * math.pi)
        phase_q = (phase_norm * (phase_levels - 1)).round().clamp(0, phase_levels - 1).to(torch.uint8)
        return mag_q, phase_q
    dev, zc = z.device, _flat(z)
    mag_q = torch.empty(z.shape, dtype=torch.uint8, device=dev)
    phase_q = torch.empty(z.shape, dtype=torch.uint8, device=dev)
    _call(dev, "smx_polar_quantize", zc.data_ptr(), mag_q.data_ptr(), phase_q.data_ptr(), zc.numel(), int(mag_bits),
          int(phase_bits), mag_min, mag_max, mwg, _stream(dev))
    return mag_q, phase_q


def polar_dequantize(mag_q: torch.Tensor, phase_q: torch.Tensor, mag_bits: int, phase_bits: int, mag_range, *,
                     max_workgroups: int = 0) -> torch.Tensor:
    """complex64 of the planes' shape: PolarQuantizer.dequantize (fft_tensor/polar_quantization.py:44-56),
        2 ** (mag_q / Lm * (mag_max - mag_min) + mag_min) * exp(i (phase_q / Lp * 2 pi - pi)).
    uint8 planes on a ROCm device with both bit counts in 1..8: smx_polar_dequantize, one launch whose workgroups build the
    256 magnitudes and 256 unit vectors in LDS and then stream 2 bytes in, 8 out, without a transcendental (the reference:
    pow, polar and eight arithmetic passes).  Everything else runs the reference's ops."""
    _check_planes("polar_dequantize", mag_q, phase_q)
    mag_min, mag_max = (float(v) for v in mag_range)
    mwg = _check_wg("polar_dequantize", max_workgroups)
    mag_levels, phase_levels = 2 ** mag_bits, 2 ** phase_bits
    if not (mag_q.dtype == torch.uint8 and phase_q.dtype == torch.uint8 and mag_q.numel() > 0
            and _codec_native(mag_q, phase_q, bits=(mag_bits, phase_bits))):
        mag_norm = mag_q.float() / (mag_levels - 1)
        log_mag = mag_norm * (mag_max - mag_min) + mag_min
        mag = 2.0 ** log_mag
        phase_norm = phase_q.float() / (phase_levels - 1)
        phase = phase_norm * 2 * math.pi - math.pi
        return torch.polar(mag, phase)
    dev, mq, pq = mag_q.device, _flat(mag_q), _flat(phase_q)
    z = torch.empty(mag_q.shape, dtype=torch.complex64, device=dev)
    _call(dev, "smx_polar_dequantize", mq.data_ptr(), pq.data_ptr(), z.data_ptr(), mq.numel(), int(mag_bits),
          int(phase_bits), mag_min, mag_max, mwg, _stream(dev))
    return z


def _log8_encode_torch(x: torch.Tensor) -> torch.Tensor:
    """LogarithmicQuantizer.log8_encode, the reference's op sequence (fft_tensor/zero_materialize.py:482-497)"""
    sign = (x >= 0).to(torch.uint8)
    magnitude = torch.abs(x)
    log_mag = torch.log2(magnitude + 1e-8)
    quantized = ((log_mag + 8) / 16 * 127).clamp(0, 127).to(torch.uint8)
    return (sign << 7) | quantized


def _log8_decode_torch(encoded: torch.Tensor) -> torch.Tensor:
    """LogarithmicQuantizer.log8_decode, the reference's op sequence (fft_tensor/zero_materialize.py:510-521)"""
    sign = ((encoded >> 7) & 1).to(torch.float32) * 2 - 1
    quantized = (encoded & 0x7F).to(torch.float32)
    log_mag = (quantized / 127) * 16 - 8
    magnitude = torch.pow(2.0, log_mag)
    return sign * magnitude


def log8_encode(x: torch.Tensor, *, max_workgroups: int = 0) -> torch.Tensor:
    """uint8 of x's shape, LogarithmicQuantizer.log8_encode:
        (x >= 0) << 7 | trunc(clamp((log2(|x| + 1e-8) + 8) / 16 * 127, 0, 127))     (so +0.0 and -0.0 both carry bit 7).
    fp32 on a ROCm device: smx_log8_encode, one launch (4 bytes in, 1 out per element; the reference: nine passes); a code
    can differ from the reference's by one where the value before truncation lies within about 1e-5 of an integer.
    Everything else runs the reference's ops.  Not differentiable."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("log8_encode: x must be a tensor")
    mwg = _check_wg("log8_encode", max_workgroups)
    if not (x.dtype == torch.float32 and x.numel() > 0 and _codec_native(x)):
        return _log8_encode_torch(x)
    dev, xc = x.device, _flat(x)
    out = torch.empty(x.shape, dtype=torch.uint8, device=dev)
    _call(dev, "smx_log8_encode", xc.data_ptr(), out.data_ptr(), xc.numel(), mwg, _stream(dev))
    return out


def log8_decode(encoded: torch.Tensor, *, max_workgroups: int = 0) -> torch.Tensor:
    """float32 of the codes' shape, LogarithmicQuantizer.log8_decode: (bit 7 ? +1 : -1) * 2 ** ((e & 127) / 127 * 16 - 8).
    uint8 on a ROCm device: smx_log8_decode, one launch that looks the 256 possible values up in an LDS table.  Everything
    else runs the reference's ops."""
    if not isinstance(encoded, torch.Tensor):
        raise TypeError("log8_decode: encoded must be a tensor")
    mwg = _check_wg("log8_decode", max_workgroups)
    if not (encoded.dtype == torch.uint8 and encoded.numel() > 0 and _codec_native(encoded)):
        return _log8_decode_torch(encoded)
    dev, ec = encoded.device, _flat(encoded)
    x = torch.empty(encoded.shape, dtype=torch.float32, device=dev)
    _call(dev, "smx_log8_decode", ec.data_ptr(), x.data_ptr(), ec.numel(), mwg, _stream(dev))
    return x


def log8_encode_complex(z: torch.Tensor, *, max_workgroups: int = 0):
    """(re_q, im_q): log8_encode of the real and of the imaginary part (LogarithmicQuantizer.compress_sparse_freq, which
    runs two strided chains).  complex64 on a ROCm device: smx_log8_encode_c64, ONE pass over the interleaved data."""
    if not (isinstance(z, torch.Tensor) and z.is_complex()):
        raise TypeError("log8_encode_complex: z must be a complex tensor")
    mwg = _check_wg("log8_encode_complex", max_workgroups)
    if not (z.dtype == torch.complex64 and z.numel() > 0 and _codec_native(z)):
        return _log8_encode_torch(z.real), _log8_encode_torch(z.imag)
    dev, zc = z.device, _flat(z)
    re_q = torch.empty(z.shape, dtype=torch.uint8, device=dev)
    im_q = torch.empty(z.shape, dtype=torch.uint8, device=dev)
    _call(dev, "smx_log8_encode_c64", zc.data_ptr(), re_q.data_ptr(), im_q.data_ptr(), zc.numel(), mwg, _stream(dev))
    return re_q, im_q


def log8_decode_complex(re_q: torch.Tensor, im_q: torch.Tensor, *, max_workgroups: int = 0) -> torch.Tensor:
    """complex64: log8_decode(re_q) + i log8_decode(im_q).  uint8 planes on a ROCm device: smx_log8_decode_c64, one launch
    that writes the interleaved tensor directly."""
    _check_planes("log8_decode_complex", re_q, im_q)
    mwg = _check_wg("log8_decode_complex", max_workgroups)
    if not (re_q.dtype == torch.uint8 and im_q.dtype == torch.uint8 and re_q.numel() > 0 and _codec_native(re_q, im_q)):
        return torch.complex(_log8_decode_torch(re_q), _log8_decode_torch(im_q))
    dev, rc, ic = re_q.device, _flat(re_q), _flat(im_q)
    z = torch.empty(re_q.shape, dtype=torch.complex64, device=dev)
    _call(dev, "smx_log8_decode_c64", rc.data_ptr(), ic.data_ptr(), z.data_ptr(), rc.numel(), mwg, _stream(dev))
    return z
