"""bf16 / fp16 activations of SpectralMixingLayer (include/smx.h smx_forward_io / smx_backward_io).

The contract is bitwise: all arithmetic is fp32 and the 2-byte input widens exactly, so for every shape and plan

    layer(x_h)          == layer_fp32(x_h.float()).to(x_h.dtype)
    grad_x (half)       == grad_x_fp32(g_h.float()).to(x_h.dtype)
    parameter gradients == the fp32 path's (fp32 parameters)
    saved spectrum xk   == the fp32 path's

on the plans with native 2-byte rows (the IO instances of k_fused, k_split_a / k_split_b) and, by construction, on the
up-cast route every other plan takes.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import TOL_PARAM, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _mods():
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import _lib, functional
    return pkg, _lib, functional


def _layer(pkg, D, F, dev, p=0.0, seed=5):
    torch.manual_seed(seed)
    layer = pkg.SpectralMixingLayer(D, num_filters=F, dropout=p).to(dev)
    with torch.no_grad():
        layer.weight_real.normal_(1.0, 0.5)
        layer.weight_imag.normal_(0.0, 0.5)
        layer.bias.normal_(0.2, 0.1)
    return layer


def _run(layer, x, g, seed=11):
    """fwd + bwd; torch.manual_seed before the forward so that a training-mode call draws the same DropoutState words"""
    x = x.detach().clone().requires_grad_(True)
    for q in layer.parameters():
        q.grad = None
    torch.manual_seed(seed)
    y = layer(x)
    y.backward(g)
    torch.cuda.synchronize()
    return (y.detach(), x.grad.detach(), layer.weight_real.grad.clone(), layer.weight_imag.grad.clone(),
            layer.bias.grad.clone())


def _same(a, b):
    """bitwise, NaN == NaN (NaN payloads are not part of the contract)"""
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb)
    ia = a.masked_fill(na, 0).view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.masked_fill(nb, 0).view(torch.int16 if b.element_size() == 2 else torch.int32)
    assert torch.equal(ia, ib), f"{(ia != ib).sum().item()} elements differ"


def _check_contract(layer, x_h, g_h):
    y, gx, gwr, gwi, gb = _run(layer, x_h, g_h)
    y32, gx32, gwr32, gwi32, gb32 = _run(layer, x_h.float(), g_h.float())
    assert y.dtype == x_h.dtype and gx.dtype == x_h.dtype
    _same(y, y32.to(x_h.dtype))
    _same(gx, gx32.to(x_h.dtype))
    for a, b in ((gwr, gwr32), (gwi, gwi32), (gb, gb32)):
        assert a.dtype == torch.float32
        _same(a, b)


CASES = [  # (B, N, D, F)        plan the case must reach
    ((8, 1024, 64, 32), "fused1"),
    ((8, 1024, 64, 200), "fused2"),
    ((32, 1024, 128, 300), "fused4"),
    ((8, 4096, 128, 128), "split"),
    ((3, 2048, 96, 256), "split"),
    ((2, 1000, 8, 4), "direct"),
    ((2, 4112, 64, 64), "sixteen"),
    ((2, 4096, 64, 600), "over512"),
    ((2, 512, 7, 4), "oddD"),
]


def _assert_plan(_lib, shape, kind, dtype):
    p = _lib.plan(*shape)
    io = {torch.bfloat16: 1, torch.float16: 2}[dtype]
    native = _lib.io_supported(*shape, io)
    if kind.startswith("fused"):
        assert (p.path, p.nsplit, p.groups, p.bands) == (_lib.SMX_PATH_DECIMATED, 1, 1, int(kind[-1])) and native
    elif kind == "split":
        assert p.path == _lib.SMX_PATH_DECIMATED and p.nsplit > 1 and p.groups == 1 and native
    elif kind == "direct":
        assert p.path == _lib.SMX_PATH_DIRECT and not native
    elif kind == "sixteen":
        assert p.path == _lib.SMX_PATH_DECIM16 and not native
    elif kind == "over512":
        assert p.path == _lib.SMX_PATH_DECIMATED and p.k > 512 and not native
    elif kind == "oddD":
        assert shape[2] % 2 == 1 and not native


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,kind", CASES, ids=[c[1] + "-" + "x".join(map(str, c[0])) for c in CASES])
def test_bitwise_contract(gpu, shape, kind, dtype):
    pkg, _lib, _ = _mods()
    _assert_plan(_lib, shape, kind, dtype)
    B, N, D, F = shape
    layer = _layer(pkg, D, F, gpu)
    torch.manual_seed(1)
    x = torch.randn(B, N, D, device=gpu).to(dtype)
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    _check_contract(layer, x, g)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(8, 1024, 64, 32), (8, 1024, 64, 200), (32, 1024, 128, 300), (8, 4096, 128, 128),
                                   (2, 1000, 8, 4)])
def test_bitwise_contract_with_fused_dropout(gpu, shape, dtype):
    pkg, _lib, _ = _mods()
    B, N, D, F = shape
    layer = _layer(pkg, D, F, gpu, p=0.25)
    layer.train()
    torch.manual_seed(2)
    x = torch.randn(B, N, D, device=gpu).to(dtype)
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    y, *_ = _run(layer, x, g)
    assert (y == 0).float().mean().item() > 0.1                 # the mask is applied
    _check_contract(layer, x, g)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(8, 1024, 64, 32), (32, 1024, 128, 300), (8, 4096, 128, 128)])
def test_saved_spectrum_and_phase_split(gpu, shape, dtype):
    """forward_raw's xk equals the fp32 path's; SPECTRUM -> INVERSE -> PARAMS equals the single fused backward"""
    _, _lib, fn = _mods()
    B, N, D, F = shape
    io = {torch.bfloat16: 1, torch.float16: 2}[dtype]
    torch.manual_seed(3)
    x = torch.randn(B, N, D, device=gpu).to(dtype)
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    wr = torch.randn(D, F, device=gpu) * 0.5 + 1
    wi = torch.randn(D, F, device=gpu) * 0.5
    b = torch.randn(D, device=gpu) * 0.1
    y, xk = fn.forward_raw(x, wr, wi, b, save_spectrum=True, io=io)
    y32, xk32 = fn.forward_raw(x.float(), wr, wi, b, save_spectrum=True)
    assert y.dtype == dtype and xk.dtype == torch.complex64
    _same(y, y32.to(dtype))
    _same(torch.view_as_real(xk), torch.view_as_real(xk32))
    gx, flat = fn.backward_raw(g, xk, wr, wi, io=io)
    gx32, flat32 = fn.backward_raw(g.float(), xk32, wr, wi)
    _same(gx, gx32.to(dtype))
    _same(flat, flat32)
    ws = torch.empty(_lib.workspace_bytes(B, N, D, F), dtype=torch.uint8, device=gpu)
    gx2, flat2 = fn.backward_raw(g, xk, wr, wi, phases=fn.PHASE_SPECTRUM, ws=ws, io=io, want_x=True)
    fn.backward_raw(g, xk, wr, wi, want_x=False, phases=fn.PHASE_PARAMS, flat=flat2, ws=ws, io=io)
    fn.backward_raw(g, xk, wr, wi, want_x=True, phases=fn.PHASE_INVERSE, grad_x=gx2, flat=flat2, ws=ws, io=io)
    torch.cuda.synchronize()
    _same(gx2, gx)
    _same(flat2, flat)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(8, 1024, 64, 32), (8, 4096, 128, 128)])
def test_direct_abi_calls(gpu, shape, dtype):
    """smx_forward_io / smx_backward_io with 2-byte device buffers: the native path itself, not the Python route"""
    _, _lib, fn = _mods()
    lib = _lib.lib()
    B, N, D, F = shape
    io = {torch.bfloat16: 1, torch.float16: 2}[dtype]
    k = min(F, N // 2)
    torch.manual_seed(4)
    x = torch.randn(B, N, D, device=gpu).to(dtype)
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    wr = torch.randn(D, F, device=gpu)
    wi = torch.randn(D, F, device=gpu)
    b = torch.randn(D, device=gpu)
    y = torch.empty_like(x)
    xk = torch.empty(B, k, D, dtype=torch.complex64, device=gpu)
    nws = _lib.workspace_bytes(B, N, D, F)
    ws = torch.empty(nws, dtype=torch.uint8, device=gpu)
    fn._prepare(gpu, N)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.smx_forward_io(x.data_ptr(), wr.data_ptr(), wi.data_ptr(), b.data_ptr(), y.data_ptr(),
                                  xk.data_ptr(), ws.data_ptr(), nws, B, N, D, F, 0, 0.0, None, None, s, io))
    gx = torch.empty_like(g)
    flat = torch.empty(2 * D * F + D, device=gpu)
    _lib.check(lib.smx_backward_io(g.data_ptr(), xk.data_ptr(), wr.data_ptr(), wi.data_ptr(), gx.data_ptr(),
                                   flat.data_ptr(), flat[D * F:].data_ptr(), flat[2 * D * F:].data_ptr(),
                                   ws.data_ptr(), nws, B, N, D, F, 7, 0.0, None, None, s, io))
    y32, xk32 = fn.forward_raw(x.float(), wr, wi, b, save_spectrum=True)
    gx32, flat32 = fn.backward_raw(g.float(), xk32, wr, wi)
    torch.cuda.synchronize()
    _same(y, y32.to(dtype))
    _same(gx, gx32.to(dtype))
    _same(flat, flat32)
    # a plan without native 2-byte rows: an error, nothing written
    x2 = torch.randn(2, 1000, 8, device=gpu).to(dtype)
    y2 = torch.full_like(x2, 7.0)
    w2 = torch.ones(8, 4, device=gpu)
    rc = lib.smx_forward_io(x2.data_ptr(), w2.data_ptr(), w2.data_ptr(), None, y2.data_ptr(), None, None, 0,
                            2, 1000, 8, 4, 0, 0.0, None, None, s, io)
    torch.cuda.synchronize()
    assert rc == -2 and b"smx_io_supported" in lib.smx_last_error()
    assert bool((y2 == 7.0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_module_cast_to_dtype(gpu, dtype):
    pkg, _, _ = _mods()
    B, N, D, F = 8, 1024, 64, 32
    ref = _layer(pkg, D, F, gpu)
    half = _layer(pkg, D, F, gpu).to(dtype)
    torch.manual_seed(6)
    x = torch.randn(B, N, D, device=gpu).to(dtype)
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    with torch.no_grad():                        # the fp32 module holds the half module's (rounded) weights
        for p32, ph in zip(ref.parameters(), half.parameters()):
            p32.copy_(ph.float())
    y, gx, gwr, gwi, gb = _run(half, x, g)
    y32, gx32, gwr32, gwi32, gb32 = _run(ref, x.float(), g.float())
    for a, b in ((y, y32), (gx, gx32), (gwr, gwr32), (gwi, gwi32), (gb, gb32)):
        assert a.dtype == dtype
        _same(a, b.to(dtype))


def test_fp16_overflow_and_nan(gpu):
    pkg, _, _ = _mods()
    B, N, D, F = 8, 1024, 64, 32
    layer = _layer(pkg, D, F, gpu)
    with torch.no_grad():                              # gain 2 on the kept low bins: |y| up to ~2 |x|
        layer.weight_real.fill_(4.0)
        layer.weight_imag.zero_()
        layer.bias.zero_()
    torch.manual_seed(7)
    n = torch.arange(N, device=gpu, dtype=torch.float32)[None, :, None]
    ph = torch.rand(B, 1, D, device=gpu) * 6.283
    x = (40000.0 * torch.cos(6.283185307 * n / N + ph) + 100.0 * torch.randn(B, N, D, device=gpu)).half()
    x[0, 5, 3] = float("nan")
    assert bool(torch.isfinite(x[1:]).all())
    g = torch.randn(B, N, D, device=gpu).half()
    y, gx, *_ = _run(layer, x, g)
    y32, gx32, *_ = _run(layer, x.float(), g.float())
    assert bool(torch.isinf(y[1:]).any()) and bool(torch.isnan(y).any())
    _same(y, y32.half())
    _same(gx, gx32.half())
    assert bool(torch.isnan(y[0, :, 3]).all()) and not bool(torch.isnan(y[1:]).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_hipgraph_capture_and_replay(gpu, dtype):
    pkg, _, _ = _mods()
    B, N, D, F = 8, 4096, 128, 128                  # split plan: four launches per direction
    layer = _layer(pkg, D, F, gpu)
    torch.manual_seed(8)
    x = torch.randn(B, N, D, device=gpu).to(dtype).requires_grad_(True)
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    y_e, gx_e, gwr_e, *_ = _run(layer, x, g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for q in layer.parameters():
                q.grad = None
            x.grad = None
            layer(x).backward(g)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    for q in layer.parameters():
        q.grad = None
    x.grad = None
    with torch.cuda.graph(graph):
        y_g = layer(x)
        y_g.backward(g)
    for q in layer.parameters():
        q.grad.zero_()
    x.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(y_g.detach(), y_e)
    _same(x.grad, gx_e)
    _same(layer.weight_real.grad, gwr_e)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_misaligned_view(gpu, dtype):
    pkg, _, _ = _mods()
    B, N, D, F = 8, 1024, 64, 32
    layer = _layer(pkg, D, F, gpu)
    torch.manual_seed(9)
    buf = torch.randn(B * N * D + 1, device=gpu).to(dtype).requires_grad_(True)
    xv = buf[1:].view(B, N, D)                      # storage offset of one element: 2-byte aligned only
    assert xv.data_ptr() % 4 == 2
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    y = layer(xv)
    y.backward(g)
    gwr = layer.weight_real.grad.clone()
    y2, gx2, gwr2, *_ = _run(layer, xv.detach().contiguous().clone(), g)
    _same(y.detach(), y2)
    _same(buf.grad[1:].view(B, N, D), gx2)
    _same(gwr, gwr2)


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)],
                         ids=["bf16", "fp16"])
def test_full_size_c2_against_the_oracle(gpu, dtype, tol):
    from oracle import spectral_oracle as so
    pkg, _, _ = _mods()
    B, N, D, F = 64, 4096, 256, 128
    layer = _layer(pkg, D, F, gpu)
    torch.manual_seed(10)
    x = torch.randn(B, N, D, device=gpu).to(dtype)
    g = torch.randn(B, N, D, device=gpu).to(dtype)
    y, gx, gwr, gwi, gb = _run(layer, x, g)
    wr, wi, bb = (p.detach().cpu().numpy() for p in (layer.weight_real, layer.weight_imag, layer.bias))
    ey = egx = 0.0
    ref_p = [np.zeros((D, F)), np.zeros((D, F)), np.zeros(D)]
    my = mgx = 0.0
    dy = dgx = 0.0
    for b0 in range(0, B, 8):                       # the oracle in batch chunks (host memory)
        xo = x[b0:b0 + 8].float().cpu().numpy()
        go = g[b0:b0 + 8].float().cpu().numpy()
        yr, _ = so.forward_closed(xo, wr, wi, bb)
        gxr, a, c, d = so.backward_closed(xo, wr, wi, go)
        for i, v in enumerate((a, c, d)):
            ref_p[i] += v
        yk = y[b0:b0 + 8].float().cpu().numpy().astype(np.float64)
        gk = gx[b0:b0 + 8].float().cpu().numpy().astype(np.float64)
        my, mgx = max(my, np.abs(yr).max()), max(mgx, np.abs(gxr).max())
        dy, dgx = max(dy, np.abs(yk - yr).max()), max(dgx, np.abs(gk - gxr).max())
    ey, egx = dy / my, dgx / mgx
    assert ey <= tol and egx <= tol, (ey, egx)
    for a, r in zip((gwr, gwi, gb), ref_p):
        assert rel_err(a.cpu().numpy(), r) <= TOL_PARAM


def test_blocks_cast_to_bf16(gpu):
    pkg, _, _ = _mods()
    B, N, D = 4, 1024, 64
    for make in (lambda: pkg.SpectralMLPBlock(D, dropout=0.0), lambda: pkg.HybridSpectralAttention(D, num_heads=4,
                                                                                                   dropout=0.0)):
        torch.manual_seed(12)
        ref = make().to(gpu).eval()
        half = make().to(gpu).eval()
        half.load_state_dict(ref.state_dict())
        half = half.to(torch.bfloat16)
        with torch.no_grad():                        # the fp32 module holds the rounded weights
            for p32, ph in zip(ref.parameters(), half.parameters()):
                p32.copy_(ph.float())
        x = torch.randn(B, N, D, device=gpu).to(torch.bfloat16)
        xh = x.clone().requires_grad_(True)
        yh = half(xh)
        yh.float().square().mean().backward()
        x32 = x.float().requires_grad_(True)
        y32 = ref(x32)
        y32.square().mean().backward()
        torch.cuda.synchronize()
        assert yh.dtype == torch.bfloat16 and bool(torch.isfinite(yh).all()) and bool(torch.isfinite(xh.grad).all())
        assert rel_err(yh.float().detach().cpu().numpy(), y32.detach().cpu().numpy()) <= 2.0 ** -5


def test_fp64_still_raises(gpu):
    _, _, fn = _mods()
    w = torch.ones(8, 4, device=gpu)
    with pytest.raises(TypeError):
        fn.spectral_mix(torch.zeros(2, 512, 8, device=gpu, dtype=torch.float64), w, w)
