"""bf16 / fp16 activations of the causal spectral convolution (include/smx.h smx_conv_forward_io /
smx_conv_backward_io, functional.rank_one_conv, fixed_spectral.causal_spectral_conv, FixedSpectralBlock).

The contract is bitwise: all arithmetic is fp32 and the 2-byte input widens exactly, so for every shape

    conv(x_h)            == conv_fp32(x_h.float(), <params>.float()).to(x_h.dtype)
    grad_x (half)        == grad_x_fp32(g_h.float()).to(x_h.dtype)
    gradient of a leaf p == the fp32 call's gradient .to(p.dtype)

on the single-launch plan (k_conv1's IO instances) and, by construction, on the up-cast route every other plan takes.
"""
import ctypes

import pytest
import torch

from conftest import TOL_ACT, TOL_PARAM, load_golden, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
IO = {torch.bfloat16: 1, torch.float16: 2}
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}     # one rounding of the output dtype


def _mods():
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import _lib, functional
    return pkg, _lib, functional


def _same(a, b):
    """bitwise, NaN == NaN (NaN payloads are not part of the contract)"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb)
    ia = a.masked_fill(na, 0).view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.masked_fill(nb, 0).view(torch.int16 if b.element_size() == 2 else torch.int32)
    assert torch.equal(ia, ib), f"{(ia != ib).sum().item()} elements differ"


class _Probe:
    """counts the native 2-byte launches: a case meant to be native must not pass on the up-cast route"""

    def __init__(self, monkeypatch, lib):
        self.n = {"smx_conv_forward_io": 0, "smx_conv_backward_io": 0}
        for name in self.n:
            f = getattr(lib, name)

            def wrap(*a, _f=f, _name=name):
                if a[-2] != 0:                     # io
                    self.n[_name] += 1
                return _f(*a)
            monkeypatch.setattr(lib, name, wrap)


def _response(n_fft, dev, seed=3):
    torch.manual_seed(seed)
    fb = n_fft // 2 + 1
    return torch.randn(fb, device=dev), torch.randn(fb, device=dev)


def _run_conv(fn, x, h_re, h_im, scale, n_fft, g, want=(True, True, True, True)):
    leaves = [t.detach().clone().requires_grad_(w) if t is not None else None
              for t, w in zip((x, h_re, h_im, scale), want)]
    y = fn.rank_one_conv(leaves[0], leaves[1], leaves[2], leaves[3], n_fft)
    if y.requires_grad:
        y.backward(g)
    torch.cuda.synchronize()
    return [y.detach()] + [None if (t is None or t.grad is None) else t.grad for t in leaves]


def _check_rank_one(fn, x_h, h_re, h_im, scale, n_fft, g_h, want=(True, True, True, True)):
    got = _run_conv(fn, x_h, h_re, h_im, scale, n_fft, g_h, want)
    ref = _run_conv(fn, x_h.float(), h_re, h_im, scale, n_fft, g_h.float(), want)
    assert got[0].dtype == x_h.dtype
    _same(got[0], ref[0].to(x_h.dtype))
    if want[0]:
        assert got[1].dtype == x_h.dtype
        _same(got[1], ref[1].to(x_h.dtype))
    for a, b in zip(got[2:], ref[2:]):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == torch.float32
            _same(a, b)


# rows against n_fft: < n_fft / 2 (PAD), = n_fft / 2, folded with PAD, folded without
ROWS = {512: (200, 256, 400, 512), 1024: (300, 512, 700, 1024), 2048: (1000, 1024, 1500, 2048)}
NATIVE = [(n, r, nj) for n in (512, 1024, 2048) for r in ROWS[n] for nj in (16, 8)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n_fft,rows,nj", NATIVE)
def test_bitwise_contract_native(gpu, monkeypatch, n_fft, rows, nj, dtype):
    _, _lib, fn = _mods()
    B, D = 4, 48                                    # 48 channels: a ragged last d-tile of the 32-channel workgroups
    with _lib.options(conv1=2 if nj == 16 else 3):  # both workgroup widths on one small shape
        assert _lib.conv_io_supported(B, rows, D, n_fft, IO[dtype])
        probe = _Probe(monkeypatch, _lib.lib())
        torch.manual_seed(n_fft + rows + nj)
        x = torch.randn(B, rows, D, device=gpu).to(dtype)
        g = torch.randn(B, rows, D, device=gpu).to(dtype)
        h_re, h_im = _response(n_fft, gpu)
        scale = torch.rand(B, D, device=gpu) + 0.5
        _check_rank_one(fn, x, h_re, h_im, scale, n_fft, g)
        assert probe.n == {"smx_conv_forward_io": 1, "smx_conv_backward_io": 1}
        _check_rank_one(fn, x, h_re, h_im, None, n_fft, g)               # no row scale
        assert probe.n == {"smx_conv_forward_io": 2, "smx_conv_backward_io": 2}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_inference_and_partial_input_grads(gpu, monkeypatch, dtype):
    _, _lib, fn = _mods()
    B, R, D, n = 8, 1024, 256, 2048
    assert _lib.conv_io_supported(B, R, D, n, IO[dtype])
    probe = _Probe(monkeypatch, _lib.lib())
    torch.manual_seed(12)
    x = torch.randn(B, R, D, device=gpu).to(dtype)
    g = torch.randn(B, R, D, device=gpu).to(dtype)
    h_re, h_im = _response(n, gpu)
    scale = torch.rand(B, D, device=gpu)
    with torch.no_grad():                           # no saved spectrum (x_spectra NULL)
        y = fn.rank_one_conv(x, h_re, h_im, scale, n)
        y32 = fn.rank_one_conv(x.float(), h_re, h_im, scale, n)
    _same(y, y32.to(dtype))
    for want in ((True, False, False, False), (False, True, True, False), (False, False, False, True),
                 (True, False, False, True)):
        _check_rank_one(fn, x, h_re, h_im, scale, n, g, want)
    assert probe.n["smx_conv_forward_io"] == 5 and probe.n["smx_conv_backward_io"] == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["n4096", "conv1_off"])
def test_bitwise_contract_up_cast_route(gpu, monkeypatch, case, dtype):
    _, _lib, fn = _mods()
    B, R, D, n = (4, 2048, 64, 4096) if case == "n4096" else (8, 1024, 256, 2048)
    with _lib.options(conv1=0 if case == "conv1_off" else 1):
        assert fn.conv_supported(B, R, D, n) and not _lib.conv_io_supported(B, R, D, n, IO[dtype])
        probe = _Probe(monkeypatch, _lib.lib())
        torch.manual_seed(13)
        x = torch.randn(B, R, D, device=gpu).to(dtype)
        g = torch.randn(B, R, D, device=gpu).to(dtype)
        h_re, h_im = _response(n, gpu)
        _check_rank_one(fn, x, h_re, h_im, torch.rand(B, D, device=gpu), n, g)
        assert probe.n == {"smx_conv_forward_io": 0, "smx_conv_backward_io": 0}


def _csc_leaves(B, T, C, K, fb, dev, dtype, seed):
    """x, kernel, gain, gate logits, g_ctx: kernel and gate in x's dtype, gain in fp32 (both kinds of leaf)"""
    torch.manual_seed(seed)
    x = torch.randn(B, T, C, device=dev).to(dtype)
    kernel = (torch.randn(K, device=dev) * 0.1).to(dtype)
    gain = torch.rand(C, device=dev) + 0.5
    logits = torch.randn(fb + 3, device=dev).to(dtype)
    g_ctx = torch.rand(B, C, device=dev).to(dtype)
    return x, kernel, gain, logits, g_ctx


def _run_csc(x, kernel, gain, logits, g_ctx, cutoff, tb, g):
    from tensor_cuda_fft_amd.fixed_spectral import causal_spectral_conv
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, kernel, gain, logits, g_ctx)]
    y = causal_spectral_conv(*leaves, cutoff, tb)
    y.backward(g)
    torch.cuda.synchronize()
    return [y.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,cutoff,native", [((8, 1024, 256, 128), None, True),     # n_fft 2048
                                                 ((8, 1024, 256, 128), 300, True),      # with the cutoff mask
                                                 ((16, 300, 256, 64), 100, True),       # n_fft 512
                                                 ((4, 1024, 63, 128), 300, False),      # odd C: spectral_filter
                                                 ((8, 200, 64, 33), None, False)])      # n_fft 256 < 512
def test_causal_spectral_conv_contract(gpu, monkeypatch, shape, cutoff, native, dtype):
    _, _lib, _ = _mods()
    B, T, C, K = shape
    from tensor_cuda_fft_amd.fixed_spectral import next_pow2
    n = next_pow2(T + K - 1)
    fb = n // 2 + 1
    assert _lib.conv_io_supported(B, T, C, n, IO[dtype]) == native
    probe = _Probe(monkeypatch, _lib.lib())
    x, kernel, gain, logits, g_ctx = _csc_leaves(B, T, C, K, fb, gpu, dtype, seed=T + C)
    g = torch.randn(B, T, C, device=gpu).to(dtype)
    got = _run_csc(x, kernel, gain, logits, g_ctx, cutoff, 8, g)
    ref = _run_csc(x.float(), kernel.float(), gain, logits.float(), g_ctx.float(), cutoff, 8, g.float())
    assert probe.n["smx_conv_forward_io"] == (1 if native else 0)
    leaves = (x, x, kernel, gain, logits, g_ctx)     # the output and each gradient: in its leaf's dtype
    for a, b, leaf in zip(got, ref, leaves):
        assert a.dtype == leaf.dtype
        _same(a, b.to(leaf.dtype))


def test_fp64_still_raises(gpu):
    _, _, fn = _mods()
    from tensor_cuda_fft_amd.fixed_spectral import causal_spectral_conv
    h = torch.ones(1025, device=gpu)
    with pytest.raises(TypeError):
        fn.rank_one_conv(torch.zeros(8, 1024, 512, device=gpu, dtype=torch.float64), h, h, None, 2048)
    with pytest.raises(TypeError):
        causal_spectral_conv(torch.zeros(2, 1024, 512, device=gpu, dtype=torch.float64),
                             torch.zeros(128, device=gpu), torch.ones(512, device=gpu))


def _oracle_conv(h, kernel, gain, logits, g_ctx, cutoff, tb, g):
    """fp64 autograd of oracle.spectral_oracle.causal_conv_port on the CPU"""
    from oracle import spectral_oracle as so
    leaves = [t.detach().cpu().double().requires_grad_(True) for t in (h, kernel, gain, logits, g_ctx)]
    y = so.causal_conv_port(*leaves[:4], leaves[4], cutoff, tb)
    y.backward(g.detach().cpu().double())
    return [y.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fixed_block_cast_to_dtype_against_the_oracle(gpu, monkeypatch, dtype):
    """FixedSpectralBlock(...).to(dtype) at fft_lm's default (8, 1024, 512, 128 taps), eval mode, fwd + bwd: the
    convolution against the fp64 port of the reference on the block's own (rounded) activations and parameters.  This
    is what the 2-byte path adds: before it, a cast block raised a dtype error in its forward."""
    pkg, _lib, _ = _mods()
    B, T, C, K, tb, cutoff = 8, 1024, 512, 128, 16, 700
    torch.manual_seed(21)
    block = pkg.FixedSpectralBlock(C, T, K, tb).to(gpu)
    with torch.no_grad():
        block.kernel.normal_(0.0, 0.05)
        block.gate_freq_logits.normal_(1.0, 1.0)
        block.gain.uniform_(0.5, 1.5)
        block.gate_ctx.weight.normal_(0.0, 0.02)
    block = block.to(dtype).eval()
    probe = _Probe(monkeypatch, _lib.lib())
    x = torch.randn(B, T, C, device=gpu).to(dtype).requires_grad_(True)
    g = torch.randn(B, T, C, device=gpu).to(dtype)
    out = block(x, cutoff)
    out.backward(g)
    torch.cuda.synchronize()
    assert probe.n == {"smx_conv_forward_io": 1, "smx_conv_backward_io": 1}
    assert out.dtype == dtype and x.grad.dtype == dtype and bool(torch.isfinite(out).all())
    for name, p in block.named_parameters():
        assert p.grad is not None and p.grad.dtype == dtype and bool(torch.isfinite(p.grad).all()), name
    # the convolution of that block, on its own layer-normed activations, against the fp64 port
    with torch.no_grad():
        h = block.ln(x)
        g_ctx = torch.sigmoid(block.gate_ctx(h.mean(dim=1)))
    got = _run_csc(h, block.kernel, block.gain, block.gate_freq_logits, g_ctx, cutoff, tb, g)
    ref = _oracle_conv(h, block.kernel, block.gain, block.gate_freq_logits, g_ctx, cutoff, tb, g)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == dtype
        tol = ULP[dtype] + (TOL_ACT if i < 2 else TOL_PARAM)
        if i == 4:                                  # logits: only the first n_fft / 2 + 1 take part
            a, b = a[:1025], b[:1025]
        e = rel_err(a.float().cpu().numpy(), b.numpy())
        assert e <= tol, (i, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reference_state_dict_loaded_then_cast(gpu, dtype):
    """a reference checkpoint (tests/golden F03: the reference module's own run) loaded, then the block cast"""
    pkg, _, _ = _mods()
    z = load_golden("F03_fixed_1x1024x8")
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd.")}
    x = torch.from_numpy(z["x"])
    B, T, C = x.shape
    K = sd["kernel"].shape[0]
    block = pkg.FixedSpectralBlock(C, T, K, int(z["transition_bins"]))
    block.load_state_dict(sd)
    block = block.to(gpu).to(dtype).eval()
    cutoff = None if int(z["cutoff"]) < 0 else int(z["cutoff"])
    xg = x.to(gpu).to(dtype).requires_grad_(True)
    y = block(xg, cutoff)
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert y.dtype == dtype and xg.grad.dtype == dtype and bool(torch.isfinite(xg.grad).all())
    # every op of the block rounds to dtype here (LayerNorm, Linear, GELU as well): a few roundings of the output
    assert rel_err(y.detach().float().cpu().numpy(), z["y"]) <= 8 * ULP[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_misaligned_view(gpu, dtype):
    _, _lib, fn = _mods()
    B, R, D, n = 8, 1024, 256, 2048
    torch.manual_seed(9)
    buf = torch.randn(B * R * D + 1, device=gpu).to(dtype)
    xv = buf[1:].view(B, R, D)                      # storage offset of one element: 2-byte aligned only
    assert xv.data_ptr() % 4 == 2
    g = torch.randn(B, R, D, device=gpu).to(dtype)
    h_re, h_im = _response(n, gpu)
    _check_rank_one(fn, xv, h_re, h_im, torch.rand(B, D, device=gpu), n, g)


def test_hipgraph_capture_and_replay_of_a_bf16_block_step(gpu):
    pkg, _, _ = _mods()
    B, T, C, K = 8, 1024, 256, 128
    torch.manual_seed(8)
    block = pkg.FixedSpectralBlock(C, T, K, 8, dropout=0.0).to(gpu).to(torch.bfloat16)
    with torch.no_grad():
        block.kernel.normal_(0.0, 0.05)
    x = torch.randn(B, T, C, device=gpu).to(torch.bfloat16).requires_grad_(True)
    g = torch.randn(B, T, C, device=gpu).to(torch.bfloat16)

    def step():
        for q in block.parameters():
            q.grad = None
        x.grad = None
        y = block(x)
        y.backward(g)
        return y

    y_e = step().detach().clone()
    gx_e, gk_e = x.grad.clone(), block.kernel.grad.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    for q in block.parameters():
        q.grad = None
    x.grad = None
    with torch.cuda.graph(graph):
        y_g = block(x)
        y_g.backward(g)
    for q in block.parameters():
        q.grad.zero_()
    x.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(y_g.detach(), y_e)
    _same(x.grad, gx_e)
    _same(block.kernel.grad, gk_e)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_direct_abi_calls(gpu, dtype):
    """smx_conv_forward_io / smx_conv_backward_io with 2-byte device buffers, io = 0 against the f32 entries, and an
    unsupported plan refused with nothing written"""
    _, _lib, fn = _mods()
    lib = _lib.lib()
    B, R, D, n = 8, 1024, 256, 2048
    io = IO[dtype]
    sh = ctypes.byref(_lib.smx_shape(B, R, D, n // 2 + 1, n, n // 2 + 1))
    wsb, saveb = fn._conv_plan(B, R, D, n)
    torch.manual_seed(4)
    x = torch.randn(B, R, D, device=gpu)
    g = torch.randn(B, R, D, device=gpu)
    h_re, h_im = _response(n, gpu)
    sc = torch.rand(B, D, device=gpu)
    ws = torch.empty(wsb, dtype=torch.uint8, device=gpu)
    fn._prepare(gpu, n)
    s = torch.cuda.current_stream().cuda_stream

    def fwd_bwd(entry_f, entry_b, xx, gg, *io_arg):
        y = torch.empty_like(xx)
        xs = torch.empty(saveb, dtype=torch.uint8, device=gpu)
        _lib.check(entry_f(sh, xx.data_ptr(), h_re.data_ptr(), h_im.data_ptr(), sc.data_ptr(), y.data_ptr(),
                           xs.data_ptr(), ws.data_ptr(), wsb, *io_arg, s))
        gx = torch.empty_like(gg)
        gh = torch.empty(2, n // 2 + 1, device=gpu)
        gs = torch.empty(B, D, device=gpu)
        _lib.check(entry_b(sh, gg.data_ptr(), xs.data_ptr(), h_re.data_ptr(), h_im.data_ptr(), sc.data_ptr(),
                           gx.data_ptr(), gh[0].data_ptr(), gh[1].data_ptr(), gs.data_ptr(), ws.data_ptr(), wsb,
                           *io_arg, s))
        torch.cuda.synchronize()
        return y, xs, gx, gh, gs

    r32 = fwd_bwd(lib.smx_conv_forward, lib.smx_conv_backward, x, g)
    r0 = fwd_bwd(lib.smx_conv_forward_io, lib.smx_conv_backward_io, x, g, 0)
    for a, b in zip(r0, r32):
        assert torch.equal(a, b)
    xh, gh_ = x.to(dtype), g.to(dtype)
    rh = fwd_bwd(lib.smx_conv_forward_io, lib.smx_conv_backward_io, xh, gh_, io)
    rr = fwd_bwd(lib.smx_conv_forward, lib.smx_conv_backward, xh.float(), gh_.float())
    _same(rh[0], rr[0].to(dtype))
    assert torch.equal(rh[1], rr[1])                                    # the saved spectrum, byte for byte
    _same(rh[2], rr[2].to(dtype))
    for a, b in zip(rh[3:], rr[3:]):
        _same(a, b)
    # misaligned 2-byte pointer: refused before any launch
    y = torch.empty(B * R * D + 2, dtype=dtype, device=gpu)
    rc = lib.smx_conv_forward_io(sh, xh.data_ptr(), h_re.data_ptr(), h_im.data_ptr(), None, y[1:].data_ptr(),
                                 None, ws.data_ptr(), wsb, io, s)
    assert rc != 0 and b"4-byte aligned" in lib.smx_last_error()
    # an unsupported plan (the three-launch n_fft 4096): an error, nothing written
    B2, R2, D2, n2 = 4, 2048, 64, 4096
    sh2 = ctypes.byref(_lib.smx_shape(B2, R2, D2, n2 // 2 + 1, n2, n2 // 2 + 1))
    wsb2, _ = fn._conv_plan(B2, R2, D2, n2)
    ws2 = torch.empty(wsb2, dtype=torch.uint8, device=gpu)
    x2 = torch.randn(B2, R2, D2, device=gpu).to(dtype)
    y2 = torch.full_like(x2, 7.0)
    h2 = torch.ones(n2 // 2 + 1, device=gpu)
    rc = lib.smx_conv_forward_io(sh2, x2.data_ptr(), h2.data_ptr(), h2.data_ptr(), None, y2.data_ptr(), None,
                                 ws2.data_ptr(), wsb2, io, s)
    torch.cuda.synchronize()
    assert rc == -2 and b"smx_conv_io_supported" in lib.smx_last_error()
    assert bool((y2 == 7.0).all())


def test_fp16_overflow_and_nan_rows(gpu):
    _, _lib, fn = _mods()
    B, R, D, n = 8, 1024, 256, 2048
    assert _lib.conv_io_supported(B, R, D, n, 2)
    torch.manual_seed(10)
    x = (torch.randn(B, R, D, device=gpu) * 1.0e4).to(torch.float16)   # large enough that y overflows fp16
    x[1, 17, :] = float("nan")                                           # a NaN row
    x[2, :, 5] = float("inf")
    g = (torch.randn(B, R, D, device=gpu) * 1.0e4).to(torch.float16)
    h_re, h_im = _response(n, gpu)
    scale = torch.rand(B, D, device=gpu) + 1.0
    got = _run_conv(fn, x, h_re, h_im, scale, n, g)
    assert bool(torch.isinf(got[0]).any()) and bool(torch.isnan(got[0]).any())
    _check_rank_one(fn, x, h_re, h_im, scale, n, g)
    xb = x.to(torch.bfloat16)
    _check_rank_one(fn, xb, h_re, h_im, scale, n, g.to(torch.bfloat16))
