"""bf16 / fp16 activations of the fused block line y = x + mix(LayerNorm(x)) (include/smx.h smx_block_forward_io /
smx_block_backward_io; reference fft_tensor/spectral_layers.py:185).

The contract is bitwise, as for the layer (tests/test_half_io_gpu.py): all arithmetic is fp32 and the 2-byte input
widens exactly, so for every shape and plan

    block(x_h)                                   == block_fp32(x_h.float()).to(x_h.dtype)
    grad_x (half)                                == grad_x_fp32(g_h.float(), x_h.float()).to(x_h.dtype)
    grad of ln_w, ln_b, w_re, w_im, bias         == the fp32 path's (fp32 parameters)
    saved spectrum xk, LayerNorm statistics      == the fp32 path's

on the shapes with native 2-byte block rows (the IO instances of k_ln_stats, k_fused_blk, k_fused mode 1 and k_ln_bwd)
and, by construction, on the up-cast route every other shape takes.
"""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, TOL_PARAM, load_golden, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IO = {torch.bfloat16: 1, torch.float16: 2}
HALF = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "H*.npz")))


def _mods():
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import _lib, functional
    return pkg, _lib, functional


def _same(a, b):
    """bitwise, NaN == NaN (NaN payloads are not part of the contract)"""
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb)
    ia = a.masked_fill(na, 0).view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.masked_fill(nb, 0).view(torch.int16 if b.element_size() == 2 else torch.int32)
    assert torch.equal(ia, ib), f"{(ia != ib).sum().item()} elements differ"


def _params(D, F, dev, seed=5, absent=False):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    lw, lb, wr, wi, b = 1.0 + 0.3 * r(D), 0.2 * r(D), 1.0 + 0.5 * r(D, F), 0.5 * r(D, F), 0.1 * r(D)
    return (None, None, wr, wi, None) if absent else (lw, lb, wr, wi, b)


def _inputs(B, N, D, offset, dev, dtype, seed=1):
    """rows with their own scale around a common offset (mean >> std where the offset is large), as
    test_block_gpu.SHAPES"""
    gen = torch.Generator().manual_seed(seed + B * 1000 + N + D)
    x = offset + (1.0 + torch.rand(B, N, 1, generator=gen)) * torch.randn(B, N, D, generator=gen)
    g = torch.randn(B, N, D, generator=gen)
    return x.to(dev).to(dtype), g.to(dev).to(dtype)


def _run(fn, x, g, params, p=0.0, seed=11, sync=None):
    """fwd + bwd through spectral_block_mix; a fresh, identically seeded DropoutState per run draws the same words"""
    x = x.detach().clone().requires_grad_(True)
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in params]
    lw, lb, wr, wi, b = leaves
    ds = None
    if p > 0.0:
        torch.manual_seed(seed)
        ds = fn.DropoutState(x.device)
    y = fn.spectral_block_mix(x, lw, lb, 1e-5, wr, wi, b, sync, dropout_p=p, drop_state=ds)
    y.backward(g)
    torch.cuda.synchronize()
    return [y.detach(), x.grad.detach()] + [None if t is None else t.grad.detach() for t in leaves]


def _check_contract(fn, x_h, g_h, params, p=0.0):
    got = _run(fn, x_h, g_h, params, p)
    ref = _run(fn, x_h.float(), g_h.float(), params, p)
    assert got[0].dtype == x_h.dtype and got[1].dtype == x_h.dtype
    _same(got[0], ref[0].to(x_h.dtype))
    _same(got[1], ref[1].to(x_h.dtype))
    for a, b in zip(got[2:], ref[2:]):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == torch.float32
            _same(a, b)
    return got


def _check_raw(fn, x_h, g_h, params, io, p=0.0):
    """the raw calls: xk and ln_stats (and everything else) against the fp32 entries on the widened input"""
    lw, lb, wr, wi, b = params
    rng = torch.tensor([1234567, 89], dtype=torch.int64, device=x_h.device) if p else None
    y, xk, st = fn.block_forward_raw(x_h, lw, lb, 1e-5, wr, wi, b, dropout_p=p, rng=rng, io=io)
    y32, xk32, st32 = fn.block_forward_raw(x_h.float(), lw, lb, 1e-5, wr, wi, b, dropout_p=p, rng=rng)
    assert y.dtype == x_h.dtype and xk.dtype == torch.complex64 and st.dtype == torch.float32
    _same(y, y32.to(x_h.dtype))
    _same(torch.view_as_real(xk), torch.view_as_real(xk32))
    _same(st, st32)
    gx, flat, lnf = fn.block_backward_raw(g_h, x_h, st, lw, xk, wr, wi, dropout_p=p, rng=rng, io=io)
    gx32, flat32, lnf32 = fn.block_backward_raw(g_h.float(), x_h.float(), st32, lw, xk32, wr, wi, dropout_p=p, rng=rng)
    torch.cuda.synchronize()
    _same(gx, gx32.to(x_h.dtype))
    _same(flat, flat32)
    _same(lnf, lnf32)
    return y, xk, st, gx, flat, lnf


NATIVE = [  # (B, N, D, F, offset), bands
    ((16, 1024, 256, 128, 0.0), 1),
    ((8, 512, 512, 256, 2.0), 2),
    ((4, 256, 1024, 64, -3.0), 1),
    ((32, 1024, 128, 300, 10.0), 4),
    ((3, 768, 40, 20, 0.5), 1),           # ragged d-tile
    # the eight- and sixteen-chunk instances of k_ln_stats / k_ln_bwd_io (tests/test_block_gpu.py ties the fp32 path to
    # the oracle at the same widths).  B = 1 is the smallest batch with the single-launch plan at each of them.
    ((1, 256, 1028, 16, 2.0), 1),         # <4, 8>, one chunk past <4, 4>: the last chunk is nearly all padding
    ((1, 512, 2048, 16, 0.0), 1),         # <4, 8> full
    ((1, 256, 4096, 16, -3.0), 1),        # <4, 16> full: the widest row
    ((33, 256, 8, 4, 0.5), 1),            # 8448 rows: a ragged second pass of the row walk
]
UPCAST = [  # (B, N, D, F, offset), why
    ((8, 4096, 128, 128, 0.0), "split"),
    ((2, 300, 24, 12, 0.0), "direct"),
    ((5, 512, 6, 3, 10.0), "D%4"),
    ((2, 512, 7, 4, 1.0), "oddD"),
]
_ids = lambda cases: ["x".join(map(str, c[0][:4])) for c in cases]


def _assert_native(_lib, shape, bands, dtype):
    p = _lib.plan(*shape[:4])
    assert (p.path, p.nsplit, p.groups, p.bands) == (_lib.SMX_PATH_DECIMATED, 1, 1, bands)
    assert _lib.block_io_supported(*shape[:4], IO[dtype])


def _assert_upcast(_lib, shape, why, dtype):
    p = _lib.plan(*shape[:4])
    assert not _lib.block_io_supported(*shape[:4], IO[dtype])
    if why == "split":
        assert p.path == _lib.SMX_PATH_DECIMATED and p.nsplit > 1
    elif why == "direct":
        assert p.path == _lib.SMX_PATH_DIRECT
    elif why == "D%4":
        assert shape[2] % 4 == 2
    else:
        assert shape[2] % 2 == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,bands", NATIVE, ids=_ids(NATIVE))
def test_bitwise_contract_native(gpu, shape, bands, dtype):
    _, _lib, fn = _mods()
    _assert_native(_lib, shape, bands, dtype)
    B, N, D, F, off = shape
    params = _params(D, F, gpu)
    x, g = _inputs(B, N, D, off, gpu, dtype)
    _check_contract(fn, x, g, params)
    _check_raw(fn, x, g, params, IO[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,why", UPCAST, ids=_ids(UPCAST))
def test_bitwise_contract_up_cast_route(gpu, shape, why, dtype):
    _, _lib, fn = _mods()
    _assert_upcast(_lib, shape, why, dtype)
    B, N, D, F, off = shape
    x, g = _inputs(B, N, D, off, gpu, dtype)
    _check_contract(fn, x, g, _params(D, F, gpu))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [c[0] for c in NATIVE] + [UPCAST[0][0], UPCAST[1][0]],
                         ids=_ids(NATIVE) + _ids(UPCAST[:2]))
def test_bitwise_contract_with_fused_dropout(gpu, shape, dtype):
    _, _lib, fn = _mods()
    B, N, D, F, off = shape
    params = _params(D, F, gpu)
    x, g = _inputs(B, N, D, off, gpu, dtype, seed=2)
    y, *_ = _check_contract(fn, x, g, params, p=0.25)
    y0, *_ = _run(fn, x, g, params)                        # the mask is applied: a quarter of y is the bare residual x
    bare, bare0 = (y == x).float().mean().item(), (y0 == x).float().mean().item()
    assert bare > 0.2 and bare - bare0 > 0.15, (bare, bare0)
    if _lib.block_io_supported(B, N, D, F, IO[dtype]):
        _check_raw(fn, x, g, params, IO[dtype], p=0.25)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [c[0] for c in NATIVE] + [c[0] for c in UPCAST], ids=_ids(NATIVE) + _ids(UPCAST))
def test_bitwise_contract_without_affine_and_bias(gpu, shape, dtype):
    _, _lib, fn = _mods()
    B, N, D, F, off = shape
    params = _params(D, F, gpu, absent=True)
    x, g = _inputs(B, N, D, off, gpu, dtype, seed=3)
    _check_contract(fn, x, g, params)
    if _lib.block_io_supported(B, N, D, F, IO[dtype]):
        _check_raw(fn, x, g, params, IO[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [NATIVE[0][0], NATIVE[1][0], NATIVE[3][0]], ids=_ids([NATIVE[0], NATIVE[1], NATIVE[3]]))
def test_phase_split_backward_equals_the_single_call(gpu, shape, dtype):
    """SPECTRUM -> PARAMS -> INVERSE with one grad_h equals the single call"""
    _, _lib, fn = _mods()
    B, N, D, F, off = shape
    io = IO[dtype]
    lw, lb, wr, wi, b = params = _params(D, F, gpu)
    x, g = _inputs(B, N, D, off, gpu, dtype, seed=4)
    y, xk, st, gx, flat, lnf = _check_raw(fn, x, g, params, io)
    ws = torch.empty(_lib.workspace_bytes(B, N, D, F), dtype=torch.uint8, device=gpu)
    gh = torch.empty(B, N, D, dtype=torch.float32, device=gpu)
    kw = dict(ws=ws, io=io, grad_h=gh)
    gx2, flat2, lnf2 = fn.block_backward_raw(g, x, st, lw, xk, wr, wi, phases=fn.PHASE_SPECTRUM, **kw)
    kw.update(grad_x=gx2, flat=flat2, ln_flat=lnf2)
    fn.block_backward_raw(g, x, st, lw, xk, wr, wi, phases=fn.PHASE_PARAMS, **kw)
    fn.block_backward_raw(g, x, st, lw, xk, wr, wi, phases=fn.PHASE_INVERSE, **kw)
    torch.cuda.synchronize()
    _same(gx2, gx)
    _same(flat2, flat)
    _same(lnf2, lnf)


class _Sync:
    """a gradient sync of one rank: runs `pre` (the PARAMS phase) where the collective would be queued"""
    mode = "overlap"

    def __init__(self):
        self.calls = 0

    def active(self):
        return True

    def all_reduce(self, flat, pre=None):
        self.calls += 1
        if pre is not None:
            pre()

        class H:
            def wait(self):
                pass
        return H()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradient_sync_phase_split_through_autograd(gpu, dtype):
    _, _lib, fn = _mods()
    B, N, D, F, off = NATIVE[0][0]
    params = _params(D, F, gpu)
    x, g = _inputs(B, N, D, off, gpu, dtype, seed=5)
    sync = _Sync()
    a = _run(fn, x, g, params, sync=sync)
    assert sync.calls == 2                                  # the filter gradients, then norm1's
    b = _run(fn, x, g, params)
    for u, v in zip(a, b):
        _same(u, v)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_direct_abi_calls(gpu, dtype):
    """smx_block_forward_io / smx_block_backward_io with 2-byte device buffers: the native path itself"""
    _, _lib, fn = _mods()
    lib = _lib.lib()
    B, N, D, F, off = NATIVE[0][0]
    io = IO[dtype]
    k = min(F, N // 2)
    lw, lb, wr, wi, b = _params(D, F, gpu, seed=6)
    x, g = _inputs(B, N, D, off, gpu, dtype, seed=6)
    y = torch.empty_like(x)
    xk = torch.empty(B, k, D, dtype=torch.complex64, device=gpu)
    st = torch.empty(B, N, 2, device=gpu)
    nws = _lib.workspace_bytes(B, N, D, F)
    ws = torch.empty(nws, dtype=torch.uint8, device=gpu)
    fn._prepare(gpu, N)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.smx_block_forward_io(x.data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-5, wr.data_ptr(), wi.data_ptr(),
                                        b.data_ptr(), y.data_ptr(), xk.data_ptr(), st.data_ptr(), ws.data_ptr(), nws,
                                        B, N, D, F, 0.0, None, None, s, io))
    gx = torch.empty_like(g)
    gh = torch.empty(B, N, D, device=gpu)
    flat = torch.empty(2 * D * F + D, device=gpu)
    lnf = torch.empty(2 * D, device=gpu)
    _lib.check(lib.smx_block_backward_io(g.data_ptr(), x.data_ptr(), st.data_ptr(), lw.data_ptr(), xk.data_ptr(),
                                         wr.data_ptr(), wi.data_ptr(), gx.data_ptr(), lnf.data_ptr(),
                                         lnf[D:].data_ptr(), flat.data_ptr(), flat[D * F:].data_ptr(),
                                         flat[2 * D * F:].data_ptr(), gh.data_ptr(), ws.data_ptr(), nws, B, N, D, F, 7,
                                         0.0, None, None, s, io))
    y32, xk32, st32 = fn.block_forward_raw(x.float(), lw, lb, 1e-5, wr, wi, b)
    gx32, flat32, lnf32 = fn.block_backward_raw(g.float(), x.float(), st32, lw, xk32, wr, wi)
    torch.cuda.synchronize()
    _same(y, y32.to(dtype))
    _same(torch.view_as_real(xk), torch.view_as_real(xk32))
    _same(st, st32)
    _same(gx, gx32.to(dtype))
    _same(flat, flat32)
    _same(lnf, lnf32)
    # io = SMX_IO_F32 through the same entries is exactly the f32 entry (grad_h ignored)
    y0 = torch.empty_like(y32)
    _lib.check(lib.smx_block_forward_io(x.float().data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-5, wr.data_ptr(),
                                        wi.data_ptr(), b.data_ptr(), y0.data_ptr(), xk.data_ptr(), st.data_ptr(),
                                        ws.data_ptr(), nws, B, N, D, F, 0.0, None, None, s, 0))
    torch.cuda.synchronize()
    _same(y0, y32)
    # a shape without native 2-byte block rows: an error, nothing written
    x2 = torch.randn(2, 1000, 8, device=gpu).to(dtype)
    y2 = torch.full_like(x2, 7.0)
    st2 = torch.full((2, 1000, 2), 7.0, device=gpu)
    w2 = torch.ones(8, 4, device=gpu)
    rc = lib.smx_block_forward_io(x2.data_ptr(), None, None, 1e-5, w2.data_ptr(), w2.data_ptr(), None, y2.data_ptr(),
                                  None, st2.data_ptr(), None, 0, 2, 1000, 8, 4, 0.0, None, None, s, io)
    torch.cuda.synchronize()
    assert rc == -2 and b"smx_block_io_supported" in lib.smx_last_error()
    assert bool((y2 == 7.0).all()) and bool((st2 == 7.0).all())


def _block(pkg, D, dev, seed=12, p=0.0):
    torch.manual_seed(seed)
    blk = pkg.SpectralMLPBlock(D, mlp_ratio=2, dropout=p).to(dev).eval()
    with torch.no_grad():
        for q in blk.parameters():
            q.add_(0.1 * torch.randn_like(q))
    return blk


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_half_module_takes_the_fused_native_op(gpu, dtype):
    pkg, _lib, fn = _mods()
    from tensor_cuda_fft_amd import spectral_layers as sl
    B, N, D = 4, 1024, 64
    blk = _block(pkg, D, gpu).to(dtype)
    x = torch.randn(B, N, D, device=gpu).to(dtype).requires_grad_(True)
    assert blk._fusable(x)
    seen = []
    orig_mix, orig_sup, orig_apply = sl.spectral_block_mix, _lib.block_io_supported, fn._SpectralBlockMix.apply
    sl.spectral_block_mix = lambda *a, **k: (seen.append("mix"), orig_mix(*a, **k))[1]
    _lib.block_io_supported = lambda *a: (seen.append(("sup", a[-1])), orig_sup(*a))[1]
    fn._SpectralBlockMix.apply = staticmethod(lambda *a: (seen.append(("apply", a[0].dtype)), orig_apply(*a))[1])
    fn._block_io_cache.clear()
    try:
        y = blk(x)
        y.float().square().mean().backward()
        torch.cuda.synchronize()
    finally:
        sl.spectral_block_mix, _lib.block_io_supported, fn._SpectralBlockMix.apply = orig_mix, orig_sup, orig_apply
    assert seen == ["mix", ("sup", IO[dtype]), ("apply", dtype)]          # the 2-byte x itself reaches the op
    assert y.dtype == dtype and x.grad.dtype == dtype
    assert all(q.grad is not None and q.grad.dtype == dtype for q in blk.parameters())
    blk.fuse_norm = False
    assert not blk._fusable(x)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_first_line_of_the_half_module_is_the_fp32_module_cast(gpu, dtype):
    """the first residual line of the half module == the fp32 module holding the rounded weights, cast to the dtype"""
    pkg, _, fn = _mods()
    B, N, D = 4, 1024, 64
    ref = _block(pkg, D, gpu)
    half = _block(pkg, D, gpu).to(dtype)
    with torch.no_grad():
        for p32, ph in zip(ref.parameters(), half.parameters()):
            p32.copy_(ph.float())
    x = (0.5 + torch.randn(B, N, D, device=gpu)).to(dtype)
    g = torch.randn(B, N, D, device=gpu).to(dtype)

    def first_line(blk, xin, gin):
        for q in blk.parameters():
            q.grad = None
        xin = xin.detach().clone().requires_grad_(True)
        sm, n1 = blk.spectral_mix, blk.norm1
        assert blk._fusable(xin)
        y = fn.spectral_block_mix(xin, n1.weight, n1.bias, n1.eps, sm.weight_real, sm.weight_imag, sm.bias)
        y.backward(gin)
        torch.cuda.synchronize()
        return [y.detach(), xin.grad] + [q.grad for q in (n1.weight, n1.bias, sm.weight_real, sm.weight_imag, sm.bias)]

    a = first_line(half, x, g)
    b = first_line(ref, x.float(), g.float())
    for u, v in zip(a, b):
        assert u.dtype == dtype
        _same(u, v.to(dtype))
    # and the whole block stays close to the fp32 block (the MLP half is torch's, in the half dtype)
    with torch.no_grad():
        yh, y32 = half(x), ref(x.float())
    assert rel_err(yh.float().cpu().numpy(), y32.cpu().numpy()) <= 2.0 ** -5


def test_fp16_overflow_and_nan(gpu):
    _, _lib, fn = _mods()
    B, N, D, F = 8, 1024, 64, 32
    assert _lib.block_io_supported(B, N, D, F, 2)
    lw, lb = torch.full((D,), 60000.0, device=gpu), torch.zeros(D, device=gpu)
    wr, wi, b = torch.full((D, F), 2.0, device=gpu), torch.zeros(D, F, device=gpu), torch.zeros(D, device=gpu)
    torch.manual_seed(7)
    n = torch.arange(N, device=gpu, dtype=torch.float32)[None, :, None]
    d = torch.arange(D, device=gpu, dtype=torch.float32)[None, None, :]
    # a slow wave along the sequence whose amplitude grows with the channel: LayerNorm(x) ~ +-1.7 at the outer channels,
    # times gamma = 60000 and a filter gain of 2 on the kept bins -> |y| up to 1.2e5, past 65504
    x = ((d - D / 2) / D * torch.cos(6.283185307 * n / N) + 0.01 * torch.randn(B, N, D, device=gpu)).half()
    x[0, 5, 3] = float("nan")
    assert bool(torch.isfinite(x[1:]).all())
    g = torch.randn(B, N, D, device=gpu).half()
    params = (lw, lb, wr, wi, b)
    y, gx, *_ = _run(fn, x, g, params)
    y32, gx32, *_ = _run(fn, x.float(), g.float(), params)
    assert bool(torch.isinf(y[1:]).any()) and bool(torch.isnan(y).any())
    assert not bool(torch.isinf(y32[1:]).any())            # the overflow is the fp16 store's
    _same(y, y32.half())
    _same(gx, gx32.half())
    assert not bool(torch.isnan(y[1:]).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_hipgraph_capture_and_replay(gpu, dtype):
    _, _lib, fn = _mods()
    B, N, D, F, off = NATIVE[1][0]
    params = [t.requires_grad_(True) for t in _params(D, F, gpu)]
    x, g = _inputs(B, N, D, off, gpu, dtype, seed=8)
    x.requires_grad_(True)
    leaves = [x] + params

    def step():
        y = fn.spectral_block_mix(x, params[0], params[1], 1e-5, params[2], params[3], params[4])
        y.backward(g)
        return y

    def clear():
        for t in leaves:
            t.grad = None

    y_e = step().detach().clone()
    torch.cuda.synchronize()
    eager = [t.grad.clone() for t in leaves]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            clear()
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    clear()
    with torch.cuda.graph(graph):
        y_g = step()
    for t in leaves:
        t.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(y_g.detach(), y_e)
    for t, e in zip(leaves, eager):
        _same(t.grad, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_misaligned_view(gpu, dtype):
    _, _lib, fn = _mods()
    B, N, D, F, off = NATIVE[0][0]
    params = _params(D, F, gpu)
    torch.manual_seed(9)
    buf = torch.randn(B * N * D + 1, device=gpu).to(dtype).requires_grad_(True)
    xv = buf[1:].view(B, N, D)                      # storage offset of one element: 2-byte aligned only
    assert xv.data_ptr() % 4 == 2
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    y = fn.spectral_block_mix(xv, *params[:2], 1e-5, *params[2:])
    y.backward(g)
    torch.cuda.synchronize()
    y2, gx2, *_ = _run(fn, xv.detach().contiguous().clone(), g, params)
    _same(y.detach(), y2)
    _same(buf.grad[1:].view(B, N, D), gx2)


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)],
                         ids=["bf16", "fp16"])
def test_full_size_against_the_oracle(gpu, dtype, tol):
    """(64, 4096, 256, 128) against oracle.spectral_oracle.block_half_port in batch chunks: max|err| / max|ref| within
    twice the half-ulp of one rounding (2^-9 bf16, 2^-12 fp16), as the layer's full-size test"""
    from oracle import spectral_oracle as so
    _, _lib, fn = _mods()
    B, N, D, F = 64, 4096, 256, 128
    assert _lib.block_io_supported(B, N, D, F, IO[dtype])
    params = _params(D, F, gpu, seed=10)
    x, g = _inputs(B, N, D, 0.5, gpu, dtype, seed=10)
    got = _run(fn, x, g, params)
    y, gx = got[0], got[1]
    cpu = [t.cpu() for t in params]
    ref_p = [np.zeros(t.shape) for t in cpu]
    my = mgx = dy = dgx = 0.0
    for b0 in range(0, B, 8):                       # the oracle in batch chunks (host memory)
        r = so.block_half_port(x[b0:b0 + 8].float().cpu(), cpu[0], cpu[1], 1e-5, cpu[2], cpu[3], cpu[4],
                               g[b0:b0 + 8].float().cpu())
        for acc, v in zip(ref_p, r[2:]):
            acc += v.numpy().astype(np.float64)
        yr, gxr = r[0].numpy().astype(np.float64), r[1].numpy().astype(np.float64)
        yk = y[b0:b0 + 8].float().cpu().numpy().astype(np.float64)
        gk = gx[b0:b0 + 8].float().cpu().numpy().astype(np.float64)
        my, mgx = max(my, np.abs(yr).max()), max(mgx, np.abs(gxr).max())
        dy, dgx = max(dy, np.abs(yk - yr).max()), max(dgx, np.abs(gk - gxr).max())
    ey, egx = dy / my, dgx / mgx
    print(f"full size {dtype}: err y {ey:.3e} grad_x {egx:.3e} (bound {tol:.3e})")
    assert ey <= tol and egx <= tol, (ey, egx)
    for a, r in zip(got[2:], ref_p):
        e = rel_err(a.cpu().numpy(), r)
        print(f"  parameter gradient err {e:.3e}")
        assert e <= TOL_PARAM


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", [n for n in HALF if n[:3] in ("H01", "H02", "H03", "H04", "H05", "H06")])
def test_goldens_cast_to_the_dtype(gpu, name, dtype):
    """H01-H06 with x and g cast: the result equals the fp32 op on the cast inputs, then cast"""
    _, _, fn = _mods()
    z = load_golden(name)
    t = lambda k: torch.from_numpy(z[k]).to(gpu)
    params = tuple(t(k) for k in ("ln_weight", "ln_bias", "weight_real", "weight_imag", "bias"))
    _check_contract(fn, t("x").to(dtype), t("g").to(dtype), params)
