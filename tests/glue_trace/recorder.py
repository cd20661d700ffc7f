"""Trace of every native call the Python glue makes (functional.py and the call sites of wirtinger_ops.py,
fixed_spectral.py, streaming.py), the companion of tests/api_trace one level up: the scenarios below drive the public
functions over every route of the glue, and each call that reaches libsmx.so is written as one line -- entry point,
return code, every argument.  tests/glue_trace/expected.txt was recorded from the glue BEFORE it was given shared
helpers; tests/test_glue_trace_gpu.py compares line for line, so a refactor of the glue that changes a call, its
order, an argument, an allocation or an error text changes a line.

How an argument prints (by the entry's declared signature, _lib._SIGS):
  int / float / bool     repr of the Python value handed to ctypes
  None                   null
  smx_shape, smx_plan    its fields (a structure behind byref prints as it is AFTER the call)
  byref(size_t)          the value written
  the stream argument    S when it equals torch's current raw stream at the call, else S?
  pointer                name+offset when it lies in the storage of a tensor the scenario names (its inputs, outputs
                         and .grads; first name wins), else tN+offset: the storage of an unnamed tensor (workspace,
                         saved spectrum, a copy _dense made ...), N numbering those storages in order of first
                         appearance in the scenario; uN+0 for an address in no storage (an empty tensor's)
  return code            as it is; the two counters smx_options_epoch / smx_tables_epoch, whose value depends on what
                         the process did before, as e+N: the distance from the scenario's first reading of that counter

While a scenario runs, the recorder keeps the storage of every tensor whose data_ptr() is taken alive (it wraps
torch.Tensor.data_ptr for that).  No address that reaches the library is therefore reused within a scenario, and an
address says which tensor was meant whatever state the caching allocator was left in by the tests that ran before.

Each scenario starts from release_workspaces(), every memo cleared, an emptied allocator cache and torch.manual_seed,
and is run twice -- the first run takes whatever is initialised lazily (twiddle tables, BLAS workspaces), the second
is the one recorded.  It ends with the exception it raised, if any, and with the bytes it asked of torch's allocator
(allocated_bytes.all.allocated), so an added copy or up-cast shows while a zero-byte placeholder does not.

    python tests/glue_trace/recorder.py OUT.txt        # record (on the GPU)
"""
import bisect
import ctypes
import os
import sys

import torch

NO_STREAM = ("smx_options_default", "smx_options_push", "smx_diag_clock", "smx_rng_next")


def _mods():
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import _lib, functional
    return pkg, _lib, functional


def _fields(s) -> str:
    return "(" + ",".join(str(getattr(s, n)) for n, _ in s._fields_) + ")"


class Recorder:
    """`install(monkeypatch)` replaces _lib.lib by a function that returns a proxy around the real library."""

    def __init__(self, dev):
        _, self._lib, _ = _mods()
        self.real = self._lib.lib()
        self.dev = dev
        self.calls = []                     # (name, [token ...], rc)
        self.keep = []                      # storages behind the pointers of this scenario
        self.on = False

    def install(self, monkeypatch):
        monkeypatch.setattr(self._lib, "lib", lambda: self)
        data_ptr = torch.Tensor.data_ptr

        def keeping(t):
            if self.on and t.is_cuda:
                self.keep.append(t.untyped_storage())
            return data_ptr(t)
        monkeypatch.setattr(torch.Tensor, "data_ptr", keeping)

    def __getattr__(self, name):
        fn = getattr(self.real, name)       # looked up at call time, as the glue must
        if not callable(fn) or not self.on:
            return fn

        def call(*args):
            types = self._lib._SIGS[name][1]
            pidx = [i for i, t in enumerate(types) if t is ctypes.c_void_p]
            sidx = pidx[-1] if pidx and name not in NO_STREAM else -1
            cur = torch._C._cuda_getCurrentRawStream(self.dev.index)
            toks = []
            for i, a in enumerate(args):
                if i == sidx and a is not None:
                    toks.append("S" if a == cur else "S?")
                elif a is None:
                    toks.append("null")
                elif hasattr(a, "_obj") or isinstance(a, ctypes.Structure):
                    toks.append(("O", getattr(a, "_obj", a)))
                elif i in pidx:
                    toks.append(("P", int(a)))
                else:
                    toks.append(repr(a))
            rc = fn(*args)
            toks = [(_fields(t[1]) if isinstance(t[1], ctypes.Structure) else "->" + str(t[1].value))
                    if isinstance(t, tuple) and t[0] == "O" else t for t in toks]
            self.calls.append((name, toks, rc))
            return rc
        return call

    def lines(self, named: dict):
        """the calls so far as text, pointers resolved against `named` (name -> tensor); clears the log"""
        spans = []
        for name, t in named.items():
            if isinstance(t, torch.Tensor) and t.is_cuda:
                st = t.untyped_storage()
                if st.nbytes() > 0:
                    spans.append((st.data_ptr(), st.nbytes(), name))
        kept = sorted({(st.data_ptr(), st.nbytes()) for st in self.keep if st.nbytes() > 0})
        bases, loose, first, out = {}, {}, {}, []
        for name, toks, rc in self.calls:
            txt = []
            for t in toks:
                if not isinstance(t, tuple):
                    txt.append(t)
                    continue
                p = t[1]
                hit = next((s for s in spans if s[0] <= p < s[0] + s[1]), None)
                i = bisect.bisect_right(kept, (p, 1 << 62)) - 1
                if hit is not None:
                    txt.append(f"{hit[2]}+{p - hit[0]}")
                elif i >= 0 and p < kept[i][0] + kept[i][1]:
                    txt.append(f"t{bases.setdefault(kept[i][0], len(bases) + 1)}+{p - kept[i][0]}")
                else:
                    txt.append(f"u{loose.setdefault(p, len(loose) + 1)}+0")
            res = f"e+{rc - first.setdefault(name, rc)}" if name.endswith("_epoch") else repr(rc)
            out.append(f"{name}({', '.join(txt)}) -> {res}")
        self.calls, self.keep = [], []
        return out


# ---- scenarios ---------------------------------------------------------------------------------------------------
class _Sync:
    """a gradient sync of one rank (tests/test_block_half_io_gpu.py): runs `pre` where the collective would be queued"""

    def __init__(self, mode):
        self.mode = mode

    def active(self):
        return True

    def all_reduce(self, flat, pre=None):
        if pre is not None:
            pre()

        class H:
            def wait(self):
                pass
        return H()


class _Env:
    """what a scenario works with: the modules, the device, and run() = forward, backward, the tensors by name"""

    def __init__(self, dev):
        self.pkg, self.lib, self.fn = _mods()
        self.dev = dev

    def randn(self, *shape, dtype=torch.float32):
        return torch.randn(*shape, device=self.dev, dtype=dtype)

    def c64(self, *shape):
        return torch.randn(*shape, device=self.dev, dtype=torch.complex64)

    def run(self, call, req=None, **inputs):
        """call(**inputs) with the inputs named in `req` (default: every floating tensor) requiring grad, then
        backward with randn upstream gradients when anything requires one"""
        named = {}
        leaves = {}
        for k, v in inputs.items():
            if isinstance(v, torch.Tensor) and (v.is_floating_point() or v.is_complex()):
                v = v.detach().requires_grad_(k in req if req is not None else True)
            leaves[k] = v
            named[k] = v
        y = call(**leaves)
        outs = list(y) if isinstance(y, (tuple, list)) else [y]
        for i, o in enumerate(outs):
            named[f"y{i}"] = o
        live = [o for o in outs if o.requires_grad]
        if live:
            gs = [torch.randn_like(o) for o in live]
            for i, g in enumerate(gs):
                named[f"g{i}"] = g
            torch.autograd.backward(live, gs)
        for k, v in leaves.items():
            if isinstance(v, torch.Tensor) and v.grad is not None:
                named[k + ".grad"] = v.grad
        return named


SCENARIOS = []          # (title, plan shape or None, options dict, body(env) -> named tensors)


def scenario(title, plan=None, **opts):
    def deco(f):
        SCENARIOS.append((title, plan, opts, f))
        return f
    return deco


def _mix_inputs(e, B, N, D, F, dtype=torch.float32, bias=True, pdtype=torch.float32):
    d = dict(x=e.randn(B, N, D).to(dtype), weight_real=(1.0 + 0.5 * e.randn(D, F)).to(pdtype),
             weight_imag=(0.5 * e.randn(D, F)).to(pdtype))
    if bias:
        d["bias"] = (0.1 * e.randn(D)).to(pdtype)
    return d


def _mix(title, shape, dtype=torch.float32, bias=True, req=None, no_grad=False, dropout=0.0, sync=None, opts=None,
         pdtype=torch.float32):
    def body(e):
        kw = dict(sync=sync)
        if dropout:
            kw.update(dropout_p=dropout, drop_state=e.fn.DropoutState(e.dev))
        call = lambda **t: e.fn.spectral_mix(t["x"], t["weight_real"], t["weight_imag"], t.get("bias"), **kw)
        inputs = _mix_inputs(e, *shape, dtype=dtype, bias=bias, pdtype=pdtype)
        if no_grad:
            with torch.no_grad():
                return e.run(call, req=(), **inputs)
        return e.run(call, req=req, **inputs)
    SCENARIOS.append((f"spectral_mix {title} {shape}", shape, opts or {}, body))


S1, S2 = (2, 256, 8, 4), (8, 1024, 64, 200)
_mix("decimated, one band", S1)
_mix("decimated, two bands", S2)
_mix("residue-split", (8, 4096, 128, 128), opts=dict(nsplit=2))
_mix("residue-split, small", S2, opts=dict(nsplit=2))
_mix("four-step", (1, 2048, 8, 1024))
_mix("direct", (2, 1000, 8, 4))
_mix("sixteen-row", (2, 272, 8, 4))
_mix("odd-D pad", (4, 1024, 65, 8))
_mix("N % 16 == 8", (8, 520, 64, 8))
_mix("N % 16 == 8, dropout", (8, 520, 64, 8), dropout=0.25)
_mix("no bias", S1, bias=False)
_mix("no bias, two bands", S2, bias=False)
_mix("dropout", S2, dropout=0.25)
_mix("dropout, direct", (2, 1000, 8, 4), dropout=0.25)
_mix("no_grad", S2, no_grad=True)
_mix("only x requires grad", S2, req=("x",))
_mix("only the weights require grad", S2, req=("weight_real", "weight_imag", "bias"))
_mix("only the bias requires grad", S1, req=("bias",))
_mix("pack buffer", (8, 4096, 256, 200))
_mix("bf16 native", S2, dtype=torch.bfloat16)
_mix("fp16 native", S2, dtype=torch.float16)
_mix("fp16 native, fp16 parameters", S2, dtype=torch.float16, pdtype=torch.float16)
_mix("bf16 native, dropout, no bias", S2, dtype=torch.bfloat16, dropout=0.25, bias=False)
_mix("bf16 up-cast", (2, 1000, 8, 4), dtype=torch.bfloat16)
_mix("fp16 up-cast", (2, 1000, 8, 4), dtype=torch.float16)
for _mode in ("overlap", "fused"):
    _mix(f"sync {_mode}", S2, sync=_Sync(_mode))
    _mix(f"sync {_mode}, x frozen", S2, sync=_Sync(_mode), req=("weight_real", "weight_imag", "bias"))
    _mix(f"sync {_mode}, weights frozen", S2, sync=_Sync(_mode), req=("x",))
    _mix(f"sync {_mode}, bf16, dropout", S2, sync=_Sync(_mode), dtype=torch.bfloat16, dropout=0.25)


@scenario("spectral_mix fp32 view at a 4-byte storage offset", S1)
def _(e):
    base = e.randn(2 * 256 * 8 + 1)
    d = _mix_inputs(e, *S1)
    d.pop("x")
    n = e.run(lambda **t: e.fn.spectral_mix(base[1:].view(2, 256, 8), t["weight_real"], t["weight_imag"], t["bias"]),
              **d)
    n["base"] = base
    return n


@scenario("spectral_mix on a side stream", S2)
def _(e):
    side = torch.cuda.Stream(device=e.dev)
    side.wait_stream(torch.cuda.current_stream(e.dev))
    d = _mix_inputs(e, *S2)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        n = e.run(lambda **t: e.fn.spectral_mix(t["x"], t["weight_real"], t["weight_imag"], t["bias"]), **d)
    torch.cuda.synchronize()
    return n


@scenario("spectral_mix empty batch")
def _(e):
    return e.run(lambda **t: e.fn.spectral_mix(t["x"], t["weight_real"], t["weight_imag"], t["bias"]),
                 **_mix_inputs(e, 0, 256, 8, 4))


def _block(title, shape, dtype=torch.float32, absent=(), req=None, no_grad=False, dropout=0.0, sync=None,
           pdtype=torch.float32):
    def body(e):
        B, N, D, F = shape
        d = _mix_inputs(e, B, N, D, F, dtype=dtype, pdtype=pdtype)
        d["ln_weight"] = (1.0 + 0.3 * e.randn(D)).to(pdtype)
        d["ln_bias"] = (0.2 * e.randn(D)).to(pdtype)
        for a in absent:
            d.pop(a)
        kw = dict(sync=sync)
        if dropout:
            kw.update(dropout_p=dropout, drop_state=e.fn.DropoutState(e.dev))
        call = lambda **t: e.fn.spectral_block_mix(t["x"], t.get("ln_weight"), t.get("ln_bias"), 1e-5,
                                                   t["weight_real"], t["weight_imag"], t.get("bias"), **kw)
        if no_grad:
            with torch.no_grad():
                return e.run(call, req=(), **d)
        return e.run(call, req=req, **d)
    SCENARIOS.append((f"spectral_block_mix {title} {shape}", shape, {}, body))


B1, B2 = (3, 768, 40, 20), (8, 512, 512, 256)
_block("native", B1)
_block("two bands", B2)
_block("bf16 native", B1, dtype=torch.bfloat16)
_block("fp16 native, fp16 parameters", B1, dtype=torch.float16, pdtype=torch.float16)
_block("bf16 up-cast", (2, 300, 24, 12), dtype=torch.bfloat16)
_block("fp16 up-cast, odd D", (2, 512, 7, 4), dtype=torch.float16)
_block("direct", (2, 300, 24, 12))
_block("unsupported D (composition)", (1, 64, 1026, 4))
_block("odd-D composition", (4, 1024, 65, 8))
_block("no ln_weight", B1, absent=("ln_weight",))
_block("no ln_bias", B1, absent=("ln_bias",))
_block("no bias", B1, absent=("bias",))
_block("no ln_weight, ln_bias, bias", B1, absent=("ln_weight", "ln_bias", "bias"))
_block("dropout", B1, dropout=0.25)
_block("no_grad", B1, no_grad=True)
_block("only x requires grad", B1, req=("x",))
_block("only the parameters require grad", B1, req=("ln_weight", "ln_bias", "weight_real", "weight_imag", "bias"))
for _mode in ("overlap", "fused"):
    _block(f"sync {_mode}", B1, sync=_Sync(_mode))
    _block(f"sync {_mode}, bf16", B1, sync=_Sync(_mode), dtype=torch.bfloat16)
    _block(f"sync {_mode}, fp16, no LayerNorm parameters, dropout", B1, sync=_Sync(_mode), dtype=torch.float16,
           absent=("ln_weight", "ln_bias"), dropout=0.25)


def _filter(title, B, R, D, F, n_fft=None, k=None, bias=True, row_scale=False, req=None, opts=None):
    def body(e):
        d = _mix_inputs(e, B, R, D, F, bias=bias)
        if row_scale:
            d["row_scale"] = 0.5 + torch.rand(B, D, device=e.dev)
        return e.run(lambda **t: e.fn.spectral_filter(t["x"], t["weight_real"], t["weight_imag"], t.get("bias"),
                                                      n_fft=n_fft, k=k, row_scale=t.get("row_scale")), req=req, **d)
    nf = R if n_fft is None else n_fft
    kk = min(F, nf // 2) if k is None else k
    SCENARIOS.append((f"spectral_filter {title} {(B, R, D, F, nf, kk)}", (B, R, D, F, nf, kk), opts or {}, body))


_filter("zero-padded rows", 2, 100, 8, 16, n_fft=256)
_filter("k with the Nyquist bin", 2, 256, 8, 129, k=129)
_filter("no bias, direct", 2, 100, 8, 16, bias=False)
_filter("row_scale native", 3, 1024, 8, 1025, n_fft=2048, k=1025, bias=False, row_scale=True)
_filter("row_scale as a post-multiply", 3, 1024, 8, 1025, n_fft=2048, k=1025, bias=False, row_scale=True,
        opts=dict(fourstep=0))
_filter("row_scale, frozen x", 3, 1024, 8, 1025, n_fft=2048, k=1025, bias=False, row_scale=True,
        req=("weight_real", "weight_imag", "row_scale"))
_filter("frozen x", 2, 100, 8, 16, n_fft=256, req=("weight_real", "weight_imag", "bias"))
_filter("frozen weights", 2, 100, 8, 16, n_fft=256, req=("x",))
_filter("k = 0", 2, 100, 8, 16, n_fft=256, k=0)


@scenario("pruned_rfft (2, 256, 8, 4)", (2, 256, 8, 4))
def _(e):
    return e.run(lambda x: e.fn.pruned_rfft(x, 4), req=(), x=e.randn(2, 256, 8))


@scenario("pruned_rfft of a misaligned view, k = 0 and empty")
def _(e):
    base = e.randn(2 * 256 * 8 + 1)
    n = e.run(lambda x: e.fn.pruned_rfft(base[1:].view(2, 256, 8), 4), req=(), x=base)
    n["z"] = e.fn.pruned_rfft(e.randn(2, 256, 8), 0)
    n["e"] = e.fn.pruned_rfft(e.randn(0, 256, 8), 4)
    return n


@scenario("rfft_bins default, explicit k and n_fft", (2, 100, 8, 129, 256, 129))
def _(e):
    x = e.randn(2, 100, 8)
    return dict(x=x, a=e.fn.rfft_bins(x), b=e.fn.rfft_bins(x, 5), c=e.fn.rfft_bins(x, 129, 256),
                d=e.fn.rfft_bins(x, 0))


@scenario("rfft zero-padded, with autograd", (2, 100, 8, 129, 256, 129))
def _(e):
    return e.run(lambda x: e.fn.rfft(x, 256), x=e.randn(2, 100, 8))


@scenario("rfft k bins, with autograd", (2, 256, 8, 5, 256, 5))
def _(e):
    return e.run(lambda x: e.fn.rfft(x, None, 5), x=e.randn(2, 256, 8))


@scenario("irfft default, with autograd", (2, 256, 8, 129, 256, 129))
def _(e):
    return e.run(lambda spec: e.fn.irfft(spec), spec=e.c64(2, 129, 8))


@scenario("irfft trimmed (k > n // 2 + 1) and cropped rows", (2, 40, 8, 33, 64, 33))
def _(e):
    return e.run(lambda spec: e.fn.irfft(spec, 64, 40), spec=e.c64(2, 129, 8))


@scenario("seq_fft native (2, 512, 4)")
def _(e):
    return e.run(lambda z: e.fn.seq_fft(z), z=e.c64(2, 512, 4))


@scenario("seq_fft recombination (2, 100, 5), lazily conjugated")
def _(e):
    z = e.c64(2, 100, 5)
    n = e.run(lambda z: e.fn.seq_fft(z), z=z)
    n["c"] = e.fn.seq_fft(z.conj())
    n["o"] = e.fn.seq_fft(e.c64(2, 5, 3))
    return n


@scenario("hermitian_scale")
def _(e):
    return dict(a=e.fn.hermitian_scale(256, 129, e.dev), b=e.fn.hermitian_scale(256, 129, e.dev),
                c=e.fn.hermitian_scale(255, 100, e.dev), d=e.fn.hermitian_scale(8, 0, e.dev))


def _conv(title, dtype=torch.float32, scale=True, req=None, no_grad=False, opts=None):
    B, R, D, n = 4, 200, 48, 512

    def body(e):
        d = dict(x=e.randn(B, R, D).to(dtype), h_re=e.randn(n // 2 + 1), h_im=e.randn(n // 2 + 1))
        if scale:
            d["scale"] = 0.5 + torch.rand(B, D, device=e.dev)
        call = lambda **t: e.fn.rank_one_conv(t["x"], t["h_re"], t["h_im"], t.get("scale"), n)
        if no_grad:
            with torch.no_grad():
                return e.run(call, req=(), **d)
        return e.run(call, req=req, **d)
    SCENARIOS.append((f"rank_one_conv {title} {(B, R, D, n)}", None, opts or {}, body))


_conv("fp32")
_conv("fp32, scale=None", scale=False)
_conv("fp32, no_grad", no_grad=True)
_conv("fp32, only x requires grad", req=("x",))
_conv("bf16 native", dtype=torch.bfloat16, opts=dict(conv1=2))
_conv("fp16 native, scale=None", dtype=torch.float16, scale=False, opts=dict(conv1=2))
_conv("bf16 up-cast", dtype=torch.bfloat16)
_conv("fp16 up-cast, conv1 off", dtype=torch.float16, opts=dict(conv1=0))


def _response(title, logits, mask, req=None):
    def body(e):
        d = dict(kernel=e.randn(16))
        if logits:
            d["gate_logits"] = e.randn(140)
        if mask:
            d["mask"] = torch.rand(129, device=e.dev)
        return e.run(lambda **t: e.fn.conv_response(t["kernel"], t.get("gate_logits"), t.get("mask"), 256),
                     req=req, **d)
    SCENARIOS.append((f"conv_response {title}", None, {}, body))


_response("gate_logits and mask", True, True, req=("kernel", "gate_logits"))
_response("gate_logits=None", False, True, req=("kernel",))
_response("mask=None", True, False, req=("kernel", "gate_logits"))
_response("both None", False, False, req=("kernel",))
_response("only gate_logits requires grad", True, True, req=("gate_logits",))


@scenario("conv_response, one output unused")
def _(e):
    k = e.randn(16).requires_grad_(True)
    h_re, h_im = e.fn.conv_response(k, None, None, 256)
    g = e.randn(129)
    h_im.backward(g)
    return {"kernel": k, "h_re": h_re, "h_im": h_im, "g": g, "kernel.grad": k.grad}


@scenario("phase_filter")
def _(e):
    return e.run(lambda m, p: e.fn.phase_filter(m, p, 5, 16), m=e.randn(8), p=e.randn(8))


@scenario("phase_filter, one output unused, only the phase requires grad")
def _(e):
    m, p = e.randn(8), e.randn(8).requires_grad_(True)
    w_re, w_im = e.fn.phase_filter(m, p, 5, 16)
    g = e.randn(8, 5)
    w_re.backward(g)
    return {"m": m, "p": p, "w_re": w_re, "w_im": w_im, "g": g, "p.grad": p.grad}


def _dwconv(title, bias, scale, req=None):
    def body(e):
        d = dict(x=e.randn(2, 10, 8), weight=e.randn(8, 1, 3))
        if bias:
            d["bias"] = e.randn(8)
        if scale:
            d["scale"] = e.randn(2, 8)
        return e.run(lambda **t: e.fn.causal_dwconv3(t["x"], t["weight"], t.get("bias"), t.get("scale")), req=req, **d)
    SCENARIOS.append((f"causal_dwconv3 {title}", None, {}, body))


_dwconv("bias and scale", True, True)
_dwconv("bias=None", False, True)
_dwconv("scale=None", True, False)
_dwconv("both None, only the weight requires grad", False, False, req=("weight",))


for _planar in (False, True):
    @scenario(f"spectral_layer_norm planar={_planar}")
    def _(e, planar=_planar):
        return e.run(lambda z, gamma, beta: e.fn.spectral_layer_norm(z, gamma, beta, 1e-5, planar=planar),
                     z=e.c64(2, 9, 16), gamma=e.randn(9, 16), beta=e.randn(9, 16))


@scenario("spectral_layer_norm, only gamma requires grad; empty")
def _(e):
    n = e.run(lambda z, gamma, beta: e.fn.spectral_layer_norm(z, gamma, beta, 1e-5), req=("gamma",),
              z=e.c64(2, 9, 16), gamma=e.randn(9, 16), beta=e.randn(9, 16))
    n["e"] = e.fn.spectral_layer_norm(e.c64(0, 9, 16), e.randn(9, 16), e.randn(9, 16), 1e-5, planar=True)
    return n


@scenario("planar_cmul")
def _(e):
    return e.run(lambda h, f_re, f_im: e.fn.planar_cmul(h, f_re, f_im), h=e.randn(2, 2, 9, 16), f_re=e.randn(9, 16),
                 f_im=e.randn(9, 16))


@scenario("planar_cmul, only h requires grad")
def _(e):
    return e.run(lambda h, f_re, f_im: e.fn.planar_cmul(h, f_re, f_im), req=("h",), h=e.randn(2, 2, 9, 16),
                 f_re=e.randn(9, 16), f_im=e.randn(9, 16))


@scenario("add_planar")
def _(e):
    return e.run(lambda a, p: e.fn.add_planar(a, p), a=e.c64(2, 9, 16), p=e.randn(2, 2, 9, 16))


@scenario("add_planar, only a requires grad")
def _(e):
    return e.run(lambda a, p: e.fn.add_planar(a, p), req=("a",), a=e.c64(2, 9, 16), p=e.randn(2, 2, 9, 16))


def _gate(title, absent=(), req=None, reference_gain_grad=False):
    def body(e):
        B, Fq, C = 2, 9, 8
        d = dict(x=e.c64(B, Fq, C), a=e.c64(Fq), u=e.randn(C), p=e.randn(Fq), q=e.randn(B, C),
                 m=torch.rand(Fq, device=e.dev))
        for k in absent:
            d.pop(k)
        return e.run(lambda **t: e.fn.spectral_gate(t["x"], t["a"], t.get("u"), t.get("p"), t.get("q"), t.get("m"),
                                                    reference_gain_grad=reference_gain_grad), req=req, **d)
    SCENARIOS.append((f"spectral_gate {title}", None, {}, body))


_gate("every factor")
for _k in "upqm":
    _gate(f"{_k}=None", absent=(_k,))
_gate("a alone", absent=tuple("upqm"))
_gate("reference_gain_grad", reference_gain_grad=True)
_gate("reference_gain_grad, q=None", absent=("q",), reference_gain_grad=True)
_gate("only x requires grad", req=("x",))
_gate("only u requires grad", req=("u",))


@scenario("mix_paths")
def _(e):
    return e.run(lambda r, a, b, c, w: e.fn.mix_paths(r, a, b, c, w, 0.1), r=e.randn(2, 6, 8), a=e.randn(2, 6, 8),
                 b=e.randn(2, 6, 8), c=e.randn(2, 6, 8), w=e.randn(2))


@scenario("mix_paths c=None, twice (the workspace size is asked once)")
def _(e):
    n = e.run(lambda r, a, b, w: e.fn.mix_paths(r, a, b, None, w), r=e.randn(2, 6, 8), a=e.randn(2, 6, 8),
              b=e.randn(2, 6, 8), w=e.randn(2))
    m = e.run(lambda r, a, b, w: e.fn.mix_paths(r, a, b, None, w), req=("a", "w"), r=e.randn(2, 6, 8),
              a=e.randn(2, 6, 8), b=e.randn(2, 6, 8), w=e.randn(2))
    n.update({"second." + k: v for k, v in m.items()})
    return n


def _rot(e, rows, half):
    return torch.polar(torch.ones(rows, half, device=e.dev), torch.randn(rows, half, device=e.dev))


@scenario("rope_rotate")
def _(e):
    rot = _rot(e, 12, 8)
    n = e.run(lambda x: e.fn.rope_rotate(x, rot), x=e.randn(2, 8, 16))
    n["rot"] = rot
    return n


@scenario("rope_rotate with a wider table")
def _(e):
    rot = _rot(e, 12, 16)
    n = e.run(lambda x: e.fn.rope_rotate(x, rot), x=e.randn(2, 8, 16))
    n["rot"] = rot
    return n


def _rope_norm(title, absent=(), dropout=0.0, req=None, use=(0, 1)):
    def body(e):
        rot = _rot(e, 12, 8)
        d = dict(x=e.randn(2, 8, 16), w1=e.randn(16), b1=e.randn(16), w2=e.randn(16), b2=e.randn(16))
        for k in absent:
            d.pop(k)
        ds = e.fn.DropoutState(e.dev) if dropout else None

        def call(**t):
            out = e.fn.rope_norm(t["x"], rot, t.get("w1"), t.get("b1"), t.get("w2"), t.get("b2"), 1e-5, 1e-6,
                                 dropout, ds)
            return [out[i] for i in use]
        n = e.run(call, req=req, **d)
        n["rot"] = rot
        return n
    SCENARIOS.append((f"rope_norm {title}", None, {}, body))


_rope_norm("every parameter")
_rope_norm("no affine parameters", absent=("w1", "b1", "w2", "b2"))
_rope_norm("dropout", dropout=0.25)
_rope_norm("h2 unused", use=(0,))
_rope_norm("x1 unused", use=(1,))
_rope_norm("only x requires grad", req=("x",))


def _residual_norm(title, absent=(), dropout=0.0, use=(0, 1)):
    def body(e):
        d = dict(x1=e.randn(2, 8, 16), p_in=e.randn(2, 8, 16), w3=e.randn(16), b3=e.randn(16))
        for k in absent:
            d.pop(k)
        ds = e.fn.DropoutState(e.dev) if dropout else None

        def call(**t):
            out = e.fn.residual_norm(t["x1"], t["p_in"], t.get("w3"), t.get("b3"), 1e-5, dropout, ds)
            return [out[i] for i in use]
        return e.run(call, **d)
    SCENARIOS.append((f"residual_norm {title}", None, {}, body))


_residual_norm("every parameter")
_residual_norm("no affine parameters", absent=("w3", "b3"))
_residual_norm("dropout", dropout=0.25)
_residual_norm("x2 unused", use=(1,))


def _gate_blend(title, absent=(), dropout=0.0):
    def body(e):
        d = dict(a=e.randn(2, 8, 32), v=e.randn(2, 8, 16), x2=e.randn(2, 8, 16), wg=e.randn(32), bg=e.randn(32))
        for k in absent:
            d.pop(k)
        ds = e.fn.DropoutState(e.dev) if dropout else None
        return e.run(lambda **t: e.fn.gate_blend(t["a"], t["v"], t.get("x2"), t.get("wg"), t.get("bg"), 1e-5, dropout,
                                                 ds), **d)
    SCENARIOS.append((f"gate_blend {title}", None, {}, body))


_gate_blend("with x2")
_gate_blend("x2=None", absent=("x2",))
_gate_blend("x2=None, no affine parameters, dropout", absent=("x2", "wg", "bg"), dropout=0.25)


def _ema(title, mode, init, req=None):
    def body(e):
        d = dict(chunks=e.c64(2, 5, 9), rho_logit=e.randn(9), theta_raw=e.randn(9))
        if init:
            d["init"] = e.c64(2, 9)
        return e.run(lambda **t: e.fn.ema_scan(t["chunks"], t["rho_logit"], t["theta_raw"], mode, t.get("init")),
                     req=req, **d)
    SCENARIOS.append((f"ema_scan {title}", None, {}, body))


_ema("aligned", "aligned", False)
_ema("aligned, init", "aligned", True)
_ema("polar", "polar", False)
_ema("polar, init", "polar", True)
_ema("aligned, init, only the parameters require grad", "aligned", True, req=("rho_logit", "theta_raw"))


def _ema_tokens(title, mode, make):
    def body(e):
        tokens = make(e)
        n = e.run(lambda rho_logit, theta_raw: e.fn.ema_scan_tokens(tokens, 16, rho_logit, theta_raw, mode),
                  rho_logit=e.randn(9), theta_raw=e.randn(9))
        n["tokens"] = tokens
        return n
    SCENARIOS.append((f"ema_scan_tokens {title}", None, {}, body))


_tok = lambda e, T, dtype: torch.randint(0, 256, (2, T), device=e.dev).to(dtype)
_ema_tokens("uint8", "aligned", lambda e: _tok(e, 50, torch.uint8))
_ema_tokens("int64, polar", "polar", lambda e: _tok(e, 50, torch.int64))
_ema_tokens("uint8 rows of a wider buffer (strided, no copy)", "aligned", lambda e: _tok(e, 100, torch.uint8)[:, :50])
_ema_tokens("int64 every second column (copied)", "aligned", lambda e: _tok(e, 100, torch.int64)[:, ::2])
_ema_tokens("uint8 at an odd byte offset", "aligned", lambda e: _tok(e, 100, torch.uint8)[:, 1:51])


@scenario("wirtinger_ops: WirtingerGradient and WirtingerSpectralFilter")
def _(e):
    from tensor_cuda_fft_amd import wirtinger_ops as wo
    n = e.run(lambda x_freq, w: wo.WirtingerGradient.apply(x_freq, w), x_freq=e.c64(2, 5, 8), w=e.c64(1, 5, 8))
    m = e.run(lambda x_freq, w_re, w_im: wo._FilterFn.apply(x_freq, w_re, w_im), x_freq=e.c64(2, 16, 8),
              w_re=e.randn(8, 4), w_im=e.randn(8, 4))
    k = e.run(lambda x_freq, w_re, w_im: wo._FilterFn.apply(x_freq, w_re, w_im), req=("w_re", "w_im"),
              x_freq=e.c64(2, 16, 8), w_re=e.randn(8, 4), w_im=e.randn(8, 4))
    n.update({"filter." + a: v for a, v in m.items()})
    n.update({"frozen." + a: v for a, v in k.items()})
    return n


@scenario("fixed_spectral: FrequencyConvFunc")
def _(e):
    from tensor_cuda_fft_amd import fixed_spectral as fs
    return e.run(lambda x_freq, kernel_freq, gain: fs.FrequencyConvFunc.apply(x_freq, kernel_freq, gain),
                 x_freq=e.c64(2, 9, 8), kernel_freq=e.c64(9), gain=e.randn(8))


@scenario("streaming: stream_push and stream_conv")
def _(e):
    from tensor_cuda_fft_amd import streaming as sm
    Bt, T, K, C, chunk = 2, 48, 8, 32, 4
    ln, ffn_ln = torch.nn.LayerNorm(C).to(e.dev), torch.nn.LayerNorm(C).to(e.dev)
    d = dict(h=e.randn(Bt, chunk, C), ring=e.randn(Bt, T, C), sum=e.randn(Bt, 2, C),
             pos=torch.tensor([0, 46], dtype=torch.int32, device=e.dev), taps=e.randn(K + 2 * chunk - 2),
             scale=e.randn(Bt, C), ln_w=ln.weight, ln_b=ln.bias, ffn_w=ffn_ln.weight, ffn_b=ffn_ln.bias)
    with torch.no_grad():
        d["pooled"] = sm.stream_push(d["h"], ln, d["ring"], d["sum"], d["pos"])
        d["h_out"], d["ff_in"] = sm.stream_conv(d["h"], d["ring"], d["pos"], d["taps"], d["scale"], ffn_ln, K)
    return d


# ---- the error table: one call per `raise` of the public functions ------------------------------------------------
def _errors(e):
    """[(label, thunk)]: every thunk raises before a native call is made"""
    fn, dev = e.fn, e.dev
    g = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
    c = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    z = lambda *s: torch.zeros(*s, dtype=torch.complex64, device=dev)
    ds = fn.DropoutState(dev)
    x, wr, wi, b = g(2, 256, 8), g(8, 4), g(8, 4), g(8)
    h = torch.bfloat16
    rot = z(12, 8)
    E = []
    add = lambda label, thunk: E.append((label, thunk))
    # spectral_mix
    add("mix x not a tensor", lambda: fn.spectral_mix([1.0], wr, wi))
    add("mix x on the CPU", lambda: fn.spectral_mix(c(2, 256, 8), wr, wi))
    add("mix x float64", lambda: fn.spectral_mix(g(2, 256, 8, dtype=torch.float64), wr, wi))
    add("mix weight_real not a tensor", lambda: fn.spectral_mix(x, None, wi))
    add("mix weight_real on the CPU", lambda: fn.spectral_mix(x, c(8, 4), wi))
    add("mix weight_imag bf16 under fp32 x", lambda: fn.spectral_mix(x, wr, wi.to(h)))
    add("mix bias float64", lambda: fn.spectral_mix(x, wr, wi, b.double()))
    add("mix x 2-D", lambda: fn.spectral_mix(g(256, 8), wr, wi))
    add("mix weights of two shapes", lambda: fn.spectral_mix(x, wr, g(8, 5)))
    add("mix weights 1-D", lambda: fn.spectral_mix(x, g(8), g(8)))
    add("mix weights of another D", lambda: fn.spectral_mix(x, g(6, 4), g(6, 4)))
    add("mix dropout_p = 1", lambda: fn.spectral_mix(x, wr, wi, b, None, 1.0, ds))
    add("mix dropout_p < 0", lambda: fn.spectral_mix(x, wr, wi, b, None, -0.1, ds))
    add("mix dropout without a DropoutState", lambda: fn.spectral_mix(x, wr, wi, b, None, 0.5))
    add("mix half x, weight_real on the CPU", lambda: fn.spectral_mix(x.to(h), c(8, 4), wi))
    add("mix half x, weight_imag float64", lambda: fn.spectral_mix(x.to(h), wr, wi.double()))
    add("mix bf16 x, fp16 bias", lambda: fn.spectral_mix(x.to(h), wr, wi, b.half()))
    add("mix half x, weight_real not a tensor", lambda: fn.spectral_mix(x.to(h), 3, wi))
    add("mix half x 2-D", lambda: fn.spectral_mix(g(256, 8).to(h), wr, wi))
    add("mix half x, weights of two shapes", lambda: fn.spectral_mix(x.to(h), wr, g(8, 5)))
    add("mix half x native, dropout_p = 1", lambda: fn.spectral_mix(g(8, 1024, 64).to(h), g(64, 200), g(64, 200),
                                                                    None, None, 1.0, ds))
    add("mix half x native, dropout without a DropoutState",
        lambda: fn.spectral_mix(g(8, 1024, 64).to(h), g(64, 200), g(64, 200), None, None, 0.5))
    add("mix half x up-cast, dropout_p = 1", lambda: fn.spectral_mix(g(2, 1000, 8).to(h), wr, wi, None, None, 1.0, ds))
    add("mix half x up-cast, dropout without a DropoutState",
        lambda: fn.spectral_mix(g(2, 1000, 8).to(h), wr, wi, None, None, 0.5))
    # spectral_block_mix
    lw, lb = g(8), g(8)
    blk = lambda x_=x, lw_=lw, lb_=lb, wr_=wr, wi_=wi, b_=b, p=0.0, s=None: \
        fn.spectral_block_mix(x_, lw_, lb_, 1e-5, wr_, wi_, b_, None, p, s)
    add("block x not a tensor", lambda: blk(x_=None))
    add("block x on the CPU", lambda: blk(x_=c(2, 256, 8)))
    add("block x int32", lambda: blk(x_=g(2, 256, 8, dtype=torch.int32)))
    add("block ln_weight on the CPU", lambda: blk(lw_=c(8)))
    add("block ln_bias bf16 under fp32 x", lambda: blk(lb_=lb.to(h)))
    add("block weight_real not a tensor", lambda: blk(wr_=2.0))
    add("block half x, ln_weight float64", lambda: blk(x_=x.to(h), lw_=lw.double()))
    add("block bf16 x, fp16 weight_imag", lambda: blk(x_=x.to(h), wi_=wi.half()))
    add("block half x, bias on the CPU", lambda: blk(x_=x.to(h), b_=c(8)))
    add("block x 2-D", lambda: blk(x_=g(256, 8)))
    add("block half x 2-D", lambda: blk(x_=g(256, 8).to(h)))
    add("block weights of two shapes", lambda: blk(wi_=g(8, 5)))
    add("block half x, weights 1-D", lambda: blk(x_=x.to(h), wr_=g(8), wi_=g(8)))
    add("block ln_weight of another length", lambda: blk(lw_=g(7)))
    add("block ln_bias 2-D", lambda: blk(lb_=g(1, 8)))
    add("block bias of another length", lambda: blk(b_=g(9)))
    add("block dropout_p = 1", lambda: blk(p=1.0, s=ds))
    add("block dropout without a DropoutState", lambda: blk(p=0.5))
    add("block half x, dropout without a DropoutState", lambda: blk(x_=g(3, 768, 40).to(h), lw_=g(40), lb_=g(40),
                                                                   wr_=g(40, 20), wi_=g(40, 20), b_=g(40), p=0.5))
    # pruned_rfft, spectral_filter, the transform pair
    add("pruned_rfft x on the CPU", lambda: fn.pruned_rfft(c(2, 256, 8), 4))
    add("pruned_rfft x bf16", lambda: fn.pruned_rfft(x.to(h), 4))
    add("pruned_rfft x not a tensor", lambda: fn.pruned_rfft(None, 4))
    add("filter x on the CPU", lambda: fn.spectral_filter(c(2, 256, 8), wr, wi))
    add("filter x bf16", lambda: fn.spectral_filter(x.to(h), wr, wi))
    add("filter weight_imag float64", lambda: fn.spectral_filter(x, wr, wi.double()))
    add("filter bias on the CPU", lambda: fn.spectral_filter(x, wr, wi, c(8)))
    add("filter x 4-D", lambda: fn.spectral_filter(g(1, 2, 256, 8), wr, wi))
    add("filter weights of another D", lambda: fn.spectral_filter(x, g(6, 4), g(6, 4)))
    add("filter n_fft < rows", lambda: fn.spectral_filter(x, wr, wi, n_fft=128))
    add("filter k > F", lambda: fn.spectral_filter(x, wr, wi, k=5))
    add("filter k < 0", lambda: fn.spectral_filter(x, wr, wi, k=-1))
    add("filter k past the Nyquist bin", lambda: fn.spectral_filter(x, g(8, 200), g(8, 200), k=130))
    add("filter row_scale float64", lambda: fn.spectral_filter(x, wr, wi, row_scale=g(2, 8).double()))
    add("filter row_scale of another shape", lambda: fn.spectral_filter(x, wr, wi, row_scale=g(8, 2)))
    add("filter row_scale with bias", lambda: fn.spectral_filter(x, wr, wi, b, row_scale=g(2, 8)))
    add("rfft_bins x on the CPU", lambda: fn.rfft_bins(c(2, 256, 8)))
    add("rfft_bins n_fft < rows", lambda: fn.rfft_bins(x, None, 128))
    add("rfft_bins k out of range", lambda: fn.rfft_bins(x, 130))
    add("rfft x float64", lambda: fn.rfft(x.double()))
    add("rfft n < rows", lambda: fn.rfft(x, 100))
    add("rfft k < 0", lambda: fn.rfft(x, None, -1))
    add("irfft spec not a tensor", lambda: fn.irfft(None))
    add("irfft spec on the CPU", lambda: fn.irfft(torch.zeros(2, 129, 8, dtype=torch.complex64)))
    add("irfft spec float32", lambda: fn.irfft(g(2, 129, 8)))
    add("irfft spec 2-D", lambda: fn.irfft(z(129, 8)))
    add("irfft n = 0", lambda: fn.irfft(z(2, 1, 8)))
    add("irfft rows > n", lambda: fn.irfft(z(2, 129, 8), 256, 300))
    add("seq_fft z not a tensor", lambda: fn.seq_fft(None))
    add("seq_fft_raw z not a tensor", lambda: fn.seq_fft_raw([1.0]))
    add("seq_fft z on the CPU", lambda: fn.seq_fft(torch.zeros(2, 8, 4, dtype=torch.complex64)))
    add("seq_fft z float32", lambda: fn.seq_fft(g(2, 8, 4)))
    add("seq_fft z 2-D", lambda: fn.seq_fft(z(8, 4)))
    # rank_one_conv, conv_response, phase_filter, causal_dwconv3
    hr, hi_ = g(257), g(257)
    xc = g(4, 200, 48)
    add("conv x on the CPU", lambda: fn.rank_one_conv(c(4, 200, 48), hr, hi_, None, 512))
    add("conv x float64", lambda: fn.rank_one_conv(xc.double(), hr, hi_, None, 512))
    add("conv h_re bf16", lambda: fn.rank_one_conv(xc, hr.to(h), hi_, None, 512))
    add("conv h_im on the CPU", lambda: fn.rank_one_conv(xc, hr, c(257), None, 512))
    add("conv h_re of another length", lambda: fn.rank_one_conv(xc, g(256), hi_, None, 512))
    add("conv scale bf16", lambda: fn.rank_one_conv(xc, hr, hi_, g(4, 48).to(h), 512))
    add("conv scale of another shape", lambda: fn.rank_one_conv(xc, hr, hi_, g(48, 4), 512))
    add("conv unsupported shape", lambda: fn.rank_one_conv(g(4, 200, 47), hr, hi_, None, 512))
    add("conv half x, unsupported shape", lambda: fn.rank_one_conv(g(4, 100, 48).to(h), g(101), g(101), None, 200))
    add("response kernel on the CPU", lambda: fn.conv_response(c(16), None, None, 256))
    add("response gate_logits float64", lambda: fn.conv_response(g(16), g(140).double(), None, 256))
    add("response gate_logits too short", lambda: fn.conv_response(g(16), g(100), None, 256))
    add("response gate_logits 2-D", lambda: fn.conv_response(g(16), g(2, 129), None, 256))
    add("response mask on the CPU", lambda: fn.conv_response(g(16), None, c(129), 256))
    add("response mask of another length", lambda: fn.conv_response(g(16), None, g(128), 256))
    add("response kernel longer than n_fft", lambda: fn.conv_response(g(300), None, None, 256))
    add("response kernel 2-D", lambda: fn.conv_response(g(2, 8), None, None, 256))
    add("phase_filter magnitude on the CPU", lambda: fn.phase_filter(c(8), g(8), 5, 16))
    add("phase_filter phase float64", lambda: fn.phase_filter(g(8), g(8).double(), 5, 16))
    add("phase_filter of two lengths", lambda: fn.phase_filter(g(8), g(7), 5, 16))
    add("phase_filter 2-D", lambda: fn.phase_filter(g(2, 4), g(2, 4), 5, 16))
    xd = g(2, 10, 8)
    add("dwconv3 x on the CPU", lambda: fn.causal_dwconv3(c(2, 10, 8), g(8, 3)))
    add("dwconv3 weight bf16", lambda: fn.causal_dwconv3(xd, g(8, 3).to(h)))
    add("dwconv3 x 2-D", lambda: fn.causal_dwconv3(g(10, 8), g(8, 3)))
    add("dwconv3 weight of another shape", lambda: fn.causal_dwconv3(xd, g(3, 8)))
    add("dwconv3 bias on the CPU", lambda: fn.causal_dwconv3(xd, g(8, 3), c(8)))
    add("dwconv3 bias of another length", lambda: fn.causal_dwconv3(xd, g(8, 3), g(7)))
    add("dwconv3 scale float64", lambda: fn.causal_dwconv3(xd, g(8, 3), None, g(2, 8).double()))
    add("dwconv3 scale of another shape", lambda: fn.causal_dwconv3(xd, g(8, 3), None, g(8, 2)))
    # the twin blocks' ops
    zz = z(2, 9, 8)
    add("gate x not a tensor", lambda: fn.spectral_gate(None, z(9)))
    add("gate a not a tensor", lambda: fn.spectral_gate(zz, None))
    add("gate x float32", lambda: fn.spectral_gate(g(2, 9, 8), z(9)))
    add("gate x on the CPU", lambda: fn.spectral_gate(torch.zeros(2, 9, 8, dtype=torch.complex64), z(9)))
    add("gate x 2-D", lambda: fn.spectral_gate(z(9, 8), z(9)))
    add("gate a float32", lambda: fn.spectral_gate(zz, g(9)))
    add("gate a of another length", lambda: fn.spectral_gate(zz, z(8)))
    add("gate u on the CPU", lambda: fn.spectral_gate(zz, z(9), c(8)))
    add("gate p float64", lambda: fn.spectral_gate(zz, z(9), None, g(9).double()))
    add("gate q of another shape", lambda: fn.spectral_gate(zz, z(9), None, None, g(8, 2)))
    add("gate m of another length", lambda: fn.spectral_gate(zz, z(9), None, None, None, g(8)))
    add("gate odd C", lambda: fn.spectral_gate(z(2, 9, 7), z(9)))
    r = g(2, 6, 8)
    add("mix_paths r on the CPU", lambda: fn.mix_paths(c(2, 6, 8), r, r, None, g(2)))
    add("mix_paths c bf16", lambda: fn.mix_paths(r, r, r, r.to(h), g(2)))
    add("mix_paths w not a tensor", lambda: fn.mix_paths(r, r, r, None, (0.5, 0.5)))
    add("mix_paths shapes differ", lambda: fn.mix_paths(r, g(2, 6, 4), r, None, g(2)))
    add("mix_paths w of another length", lambda: fn.mix_paths(r, r, r, None, g(3)))
    add("mix_paths count not a multiple of 4", lambda: fn.mix_paths(g(2, 3, 3), g(2, 3, 3), g(2, 3, 3), None, g(2)))
    add("mix_paths empty", lambda: fn.mix_paths(g(0, 8), g(0, 8), g(0, 8), None, g(2)))
    hp = g(2, 2, 9, 16)
    add("planar_cmul h on the CPU", lambda: fn.planar_cmul(c(2, 2, 9, 16), g(9, 16), g(9, 16)))
    add("planar_cmul f_im float64", lambda: fn.planar_cmul(hp, g(9, 16), g(9, 16).double()))
    add("planar_cmul h 3-D", lambda: fn.planar_cmul(g(2, 9, 16), g(9, 16), g(9, 16)))
    add("planar_cmul factors of another shape", lambda: fn.planar_cmul(hp, g(9, 8), g(9, 8)))
    add("add_planar a not a tensor", lambda: fn.add_planar(None, hp))
    add("add_planar p not a tensor", lambda: fn.add_planar(z(2, 9, 16), None))
    add("add_planar a float32", lambda: fn.add_planar(g(2, 9, 16), hp))
    add("add_planar a on the CPU", lambda: fn.add_planar(torch.zeros(2, 9, 16, dtype=torch.complex64), hp))
    add("add_planar p on the CPU", lambda: fn.add_planar(z(2, 9, 16), c(2, 2, 9, 16)))
    add("add_planar p of another shape", lambda: fn.add_planar(z(2, 9, 16), g(2, 9, 16)))
    zl = z(2, 9, 16)
    add("sln z not a tensor", lambda: fn.spectral_layer_norm(None, g(9, 16), g(9, 16), 1e-5))
    add("sln gamma not a tensor", lambda: fn.spectral_layer_norm(zl, None, g(9, 16), 1e-5))
    add("sln z on the CPU", lambda: fn.spectral_layer_norm(torch.zeros(2, 9, 16, dtype=torch.complex64), g(9, 16),
                                                            g(9, 16), 1e-5))
    add("sln z float32", lambda: fn.spectral_layer_norm(g(2, 9, 16), g(9, 16), g(9, 16), 1e-5))
    add("sln z 2-D", lambda: fn.spectral_layer_norm(z(9, 16), g(9, 16), g(9, 16), 1e-5))
    add("sln gamma on the CPU", lambda: fn.spectral_layer_norm(zl, c(9, 16), g(9, 16), 1e-5))
    add("sln beta bf16", lambda: fn.spectral_layer_norm(zl, g(9, 16), g(9, 16).to(h), 1e-5))
    add("sln gamma of another shape", lambda: fn.spectral_layer_norm(zl, g(16, 9), g(9, 16), 1e-5))
    # the enhanced block's row lines
    xe = g(2, 8, 16)
    add("rope_rotate x on the CPU", lambda: fn.rope_rotate(c(2, 8, 16), rot))
    add("rope_rotate x bf16", lambda: fn.rope_rotate(xe.to(h), rot))
    add("rope_rotate odd D", lambda: fn.rope_rotate(g(2, 8, 15), rot))
    add("rope_rotate D > 1024", lambda: fn.rope_rotate(g(1, 2, 1026), z(12, 513)))
    add("rope_rotate rotation float32", lambda: fn.rope_rotate(xe, g(12, 8)))
    add("rope_rotate table too short", lambda: fn.rope_rotate(g(2, 13, 16), rot))
    add("rope_norm x on the CPU", lambda: fn.rope_norm(c(2, 8, 16), rot, None, None, None, None, 1e-5, 1e-5))
    add("rope_norm table too short", lambda: fn.rope_norm(g(2, 13, 16), rot, None, None, None, None, 1e-5, 1e-5))
    add("rope_norm dropout_p = 1", lambda: fn.rope_norm(xe, rot, None, None, None, None, 1e-5, 1e-5, 1.0, ds))
    add("residual_norm x1 on the CPU", lambda: fn.residual_norm(c(2, 8, 16), xe, None, None, 1e-5))
    add("residual_norm p_in of another shape", lambda: fn.residual_norm(xe, g(2, 8, 18), None, None, 1e-5))
    add("residual_norm dropout_p < 0", lambda: fn.residual_norm(xe, xe, None, None, 1e-5, -1.0, ds))
    add("gate_blend v float64", lambda: fn.gate_blend(g(2, 8, 32), xe.double(), None, None, None, 1e-5))
    add("gate_blend a on the CPU", lambda: fn.gate_blend(c(2, 8, 32), xe, None, None, None, 1e-5))
    add("gate_blend a of another shape", lambda: fn.gate_blend(g(2, 8, 16), xe, None, None, None, 1e-5))
    add("gate_blend x2 of another shape", lambda: fn.gate_blend(g(2, 8, 32), xe, g(2, 8, 18), None, None, 1e-5))
    add("gate_blend dropout_p = 2", lambda: fn.gate_blend(g(2, 8, 32), xe, None, None, None, 1e-5, 2.0, ds))
    # SpectralEMA
    ch, rho, th = z(2, 5, 9), g(9), g(9)
    add("ema_scan unknown mode", lambda: fn.ema_scan(ch, rho, th, "diagonal"))
    add("ema_scan chunks not a tensor", lambda: fn.ema_scan(None, rho, th))
    add("ema_scan chunks float32", lambda: fn.ema_scan(g(2, 5, 9), rho, th))
    add("ema_scan chunks on the CPU", lambda: fn.ema_scan(torch.zeros(2, 5, 9, dtype=torch.complex64), rho, th))
    add("ema_scan rho_logit on the CPU", lambda: fn.ema_scan(ch, c(9), th))
    add("ema_scan theta_raw of another length", lambda: fn.ema_scan(ch, rho, g(8)))
    add("ema_scan init float32", lambda: fn.ema_scan(ch, rho, th, "aligned", g(2, 9)))
    add("ema_scan init of another shape", lambda: fn.ema_scan(ch, rho, th, "aligned", z(9, 2)))
    tk = torch.zeros(2, 50, dtype=torch.uint8, device=dev)
    add("ema_scan_tokens unknown mode", lambda: fn.ema_scan_tokens(tk, 16, rho, th, "x"))
    add("ema_scan_tokens chunk_len = 1", lambda: fn.ema_scan_tokens(tk, 1, rho, th))
    add("ema_scan_tokens chunk_len = 65", lambda: fn.ema_scan_tokens(tk, 65, rho, th))
    add("ema_scan_tokens tokens int32", lambda: fn.ema_scan_tokens(tk.int(), 16, rho, th))
    add("ema_scan_tokens tokens on the CPU", lambda: fn.ema_scan_tokens(tk.cpu(), 16, rho, th))
    add("ema_scan_tokens tokens 1-D", lambda: fn.ema_scan_tokens(tk[0], 16, rho, th))
    add("ema_scan_tokens rho_logit float64", lambda: fn.ema_scan_tokens(tk, 16, rho.double(), th))
    add("ema_scan_tokens theta_raw of another length", lambda: fn.ema_scan_tokens(tk, 16, rho, g(8)))
    # non-tensor cases of the remaining public functions, and the checks of the other modules' call sites
    add("filter x not a tensor", lambda: fn.spectral_filter(None, wr, wi))
    add("filter weight_real not a tensor", lambda: fn.spectral_filter(x, None, wi))
    add("rfft_bins x not a tensor", lambda: fn.rfft_bins(None))
    add("rfft x not a tensor", lambda: fn.rfft(None))
    add("conv x not a tensor", lambda: fn.rank_one_conv(None, hr, hi_, None, 512))
    add("conv h_re not a tensor", lambda: fn.rank_one_conv(xc, None, hi_, None, 512))
    add("response kernel not a tensor", lambda: fn.conv_response(None, None, None, 256))
    add("phase_filter magnitude not a tensor", lambda: fn.phase_filter(None, g(8), 5, 16))
    add("dwconv3 x not a tensor", lambda: fn.causal_dwconv3(None, g(8, 3)))
    add("dwconv3 weight not a tensor", lambda: fn.causal_dwconv3(xd, None))
    add("planar_cmul h not a tensor", lambda: fn.planar_cmul(None, g(9, 16), g(9, 16)))
    add("rope_rotate x not a tensor", lambda: fn.rope_rotate(None, rot))
    add("rope_rotate rotation not a tensor", lambda: fn.rope_rotate(xe, None))
    add("gate_blend a not a tensor", lambda: fn.gate_blend(None, xe, None, None, None, 1e-5))
    add("ema_scan rho_logit not a tensor", lambda: fn.ema_scan(ch, None, th))
    add("ema_scan init not a tensor", lambda: fn.ema_scan(ch, rho, th, "aligned", 1.0))
    add("ema_scan_tokens tokens not a tensor", lambda: fn.ema_scan_tokens(None, 16, rho, th))
    from tensor_cuda_fft_amd import fixed_spectral as fs, wirtinger_ops as wo
    add("FrequencyConvFunc x_freq not a tensor", lambda: fs.FrequencyConvFunc.apply(None, z(9), g(8)))
    add("FrequencyConvFunc x_freq float32", lambda: fs.FrequencyConvFunc.apply(g(2, 9, 8), z(9), g(8)))
    add("FrequencyConvFunc x_freq on the CPU",
        lambda: fs.FrequencyConvFunc.apply(torch.zeros(2, 9, 8, dtype=torch.complex64), z(9), g(8)))
    add("WirtingerGradient x_freq not a tensor", lambda: wo.WirtingerGradient.apply(None, z(1, 5, 8)))
    add("WirtingerGradient x_freq on the CPU",
        lambda: wo.WirtingerGradient.apply(torch.zeros(2, 5, 8, dtype=torch.complex64), z(1, 5, 8)))
    add("WirtingerGradient weight float32", lambda: wo.WirtingerGradient.apply(z(2, 5, 8), g(1, 5, 8)))
    add("WirtingerGradient weight of another shape", lambda: wo.WirtingerGradient.apply(z(2, 5, 8), z(2, 5, 8)))
    add("wirtinger filter weight.real on the CPU", lambda: wo._FilterFn.apply(z(2, 16, 8), c(8, 4), g(8, 4)))
    add("wirtinger filter weight.imag bf16", lambda: wo._FilterFn.apply(z(2, 16, 8), g(8, 4), g(8, 4).to(h)))
    return E


# ---- driver ------------------------------------------------------------------------------------------------------
def _reset(fn):
    fn.release_workspaces()
    for v in vars(fn).values():
        if isinstance(v, fn._Memo):
            v.clear()
    for name in ("_prepared", "_slow_plan_warned"):
        getattr(fn, name).clear()
    if hasattr(fn, "_MIX_WS_BYTES"):        # only for recording again from the glue expected.txt was made from:
        fn._MIX_WS_BYTES = None             # it kept these two answers in a global and a dict
        fn._enh_supported_cache.clear()
    else:
        fn._mix_ws_bytes.cache_clear()
        fn.enh_supported.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _allocated(dev) -> int:
    return torch.cuda.memory_stats(dev)["allocated_bytes.all.allocated"]


def _plan_text(lib, shape) -> str:
    if shape is None or 0 in shape[:3]:
        return "-"
    try:
        p = lib.plan(*shape) if len(shape) == 4 else lib.plan_ex(lib.smx_shape(*shape))
    except lib.SmxError as ex:
        return f"none ({ex})"
    return "path=%d k=%d L=%d bands=%d nsplit=%d workgroups=%d groups=%d" % (
        p.path, p.k, p.L, p.bands, p.nsplit, p.workgroups, p.groups)


def record(rec: Recorder) -> list:
    """run every scenario (twice: see the module docstring) and return the lines of the trace"""
    import contextlib
    import warnings
    e = _Env(rec.dev)
    out = []
    for title, shape, opts, body in SCENARIOS:
        for keep in (False, True):
            _reset(e.fn)
            torch.manual_seed(1234)
            before = _allocated(rec.dev)
            named, err = {}, None
            with (e.lib.options(**opts) if opts else contextlib.nullcontext()):
                plan = _plan_text(e.lib, shape)
                rec.on = True
                try:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        named = body(e)
                    torch.cuda.synchronize()
                except Exception as ex:                      # part of the trace: type and message
                    err = f"{type(ex).__name__}: {ex}"
                finally:
                    rec.on = False
            lines = rec.lines(named)
            delta = _allocated(rec.dev) - before
            del named
            if keep:
                out.append(f"== {title} | opts={opts or '-'} | plan {plan}")
                out += lines
                out.append(f"raised: {err or '-'}")
                out.append(f"allocated: {delta}")
    _reset(e.fn)
    out.append("== error table")
    rec.on = True
    try:
        for label, thunk in _errors(e):
            try:
                thunk()
                res = "no exception"
            except Exception as ex:
                res = f"{type(ex).__name__}: {ex}"
            out += rec.lines({})                             # the support queries some checks ask on their way
            out.append(f"{label} -> {res}")
    finally:
        rec.on = False
    return out


class _Patch:
    """monkeypatch for the command line"""

    def __init__(self):
        self.undo = []

    def setattr(self, obj, name, value):
        self.undo.append((obj, name, vars(obj).get(name, self)))
        setattr(obj, name, value)

    def close(self):
        for obj, name, value in reversed(self.undo):
            if value is self:
                delattr(obj, name)
            else:
                setattr(obj, name, value)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    rec = Recorder(torch.device("cuda:0"))
    patch = _Patch()
    rec.install(patch)
    try:
        text = record(rec)
    finally:
        patch.close()
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(text) + "\n")
    print(f"{len(text)} lines -> {sys.argv[1]}")
