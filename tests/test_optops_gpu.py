"""The per-bin channel contraction (csrc/smx_fconv.hip) and the members of optimized_ops / production_ready on the GPU.

Yardstick everywhere: the complex128 / float64 definitions of tests/optops_common.py on the CPU, max-normalised
(conftest.rel_err), under the project's bounds TOL_ACT (y, gx, grad_x) and TOL_PARAM (gw, grad_w).  Every error is
printed before it is asserted.

Which shape reaches which instance of the kernels (LB: lanes per bin of k_bc_fwd / k_bc_gw, the power of two at or above
min(ceil(Co / 2), 256); LBI: of k_bc_gx, at or above min(Ci, 256); ICH = 2 LB input channels per LDS chunk; OCH = min(8, 2 LBI)):
  (1, 1, 1, 1)        LB 1, LBI 1, one lane active
  (2, 5, 3, 5)        LB 4, odd rows: both access widths; LBI 4
  (2, 3, 2, 2)        LB 1 with Ci = ICH = 2: exactly one chunk;        (2, 3, 3, 2): Ci = ICH + 1, a second chunk
  (8, 6, 4, 6)        B = one batch tile;                               (9, 70, 17, 33): B = 9, a second tile (gw's read-modify-write)
  (3, 4, 130, 2)      65 chunks of x per tile; LBI 256 partly filled
  (2, 3, 4, 300)      LB 256 partly filled
  (2, 2, 2, 512)      LB 256 full, one output chunk;                    (2, 2, 2, 514): a second output chunk
  (1, 2, 256, 3)      LBI 256 full, one channel chunk of k_bc_gx;       (1, 2, 257, 3): a second one
  (1, 1, 513, 258)    LB 256 with Ci = ICH + 1 = 513
  (2, 3, 5, 8)        Co = OCH: one chunk of k_bc_gx;                   (2, 3, 5, 9): a second one
  (1, 70000, 2, 2)    P past 65535: 274 tiles of 256 bins
  (9, 70, 17, 33) under max_workgroups = 3: every walk takes several rounds"""
import numpy as np
import pytest
import torch

import optops_common as oc
from conftest import TOL_ACT, TOL_PARAM, load_golden, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 5, 3, 5), (2, 3, 2, 2), (2, 3, 3, 2), (8, 6, 4, 6), (9, 70, 17, 33), (3, 4, 130, 2),
          (2, 3, 4, 300), (2, 2, 2, 512), (2, 2, 2, 514), (1, 2, 256, 3), (1, 2, 257, 3), (1, 1, 513, 258), (2, 3, 5, 8),
          (2, 3, 5, 9), (1, 70000, 2, 2)]


def _err(name, got, want, tol):
    e = rel_err(got.detach().cpu().numpy(), want.numpy())
    print(f"{name}: {e:.2e} (bound {tol:.0e})")
    return e


def _operands(shape, seed=11):
    B, P, Ci, Co = shape
    g = torch.Generator().manual_seed(seed)
    return oc.crandn(g, B, P, Ci), oc.crandn(g, P, Ci, Co), oc.crandn(g, B, P, Co)


def _check_contract(gpu, shape, want=(True, True), max_workgroups=0):
    from tensor_cuda_fft_amd import functional as fn
    x, w, gy = _operands(shape)
    xd, wd = x.to(gpu).requires_grad_(want[0]), w.to(gpu).requires_grad_(want[1])
    y = fn.bin_contract(xd, wd, max_workgroups=max_workgroups)
    assert y.dtype == torch.complex64 and y.shape == gy.shape
    tag = f"bin_contract {shape} mwg={max_workgroups}"
    assert _err(tag + " y", y, oc.bin_contract_def(x, w), TOL_ACT) <= TOL_ACT
    leaves = [t for t, k in ((xd, want[0]), (wd, want[1])) if k]
    grads = dict(zip([k for k, on in (("gx", want[0]), ("gw", want[1])) if on], torch.autograd.grad(y, leaves, gy.to(gpu))))
    dx, dw = oc.bin_contract_grads_def(x, w, gy)
    if "gx" in grads:
        assert _err(tag + " gx", grads["gx"], dx, TOL_ACT) <= TOL_ACT
    if "gw" in grads:
        assert _err(tag + " gw", grads["gw"], dw, TOL_PARAM) <= TOL_PARAM


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bin_contract_forward_and_backward(gpu, shape):
    _check_contract(gpu, shape)


def test_bin_contract_under_a_workgroup_cap(gpu):
    _check_contract(gpu, (9, 70, 17, 33), max_workgroups=3)
    _check_contract(gpu, (1, 70000, 2, 2), max_workgroups=3)


def test_bin_contract_one_gradient_at_a_time(gpu):
    _check_contract(gpu, (9, 70, 17, 33), want=(True, False))
    _check_contract(gpu, (9, 70, 17, 33), want=(False, True))


def test_bin_contract_misaligned_views_and_empty_operands(gpu):
    """operands that start 8 bytes off a 16-byte boundary (the glue copies them), B = 0 and P = 0"""
    from tensor_cuda_fft_amd import functional as fn
    x, w, _ = _operands((2, 5, 3, 5))
    xb = torch.zeros(x.numel() + 1, dtype=torch.complex64, device=gpu)
    xb[1:] = x.reshape(-1).to(gpu)
    y = fn.bin_contract(xb[1:].view(x.shape), w.to(gpu))
    assert _err("misaligned x", y, oc.bin_contract_def(x, w), TOL_ACT) <= TOL_ACT
    assert fn.bin_contract(x[:0].to(gpu), w.to(gpu)).shape == (0, 5, 5)
    assert fn.bin_contract(x[:, :0].to(gpu), w[:0].to(gpu)).shape == (2, 0, 5)
    z = fn.bin_contract(x[:, :, :0].to(gpu), w[:, :0].to(gpu))
    assert z.shape == (2, 5, 5) and not z.any()


def test_raw_entries_refuse_bad_arguments(gpu):
    """NULL pointers, negative sizes, a negative max_workgroups: SMX_ERR_INVALID; sizes beyond the limits:
    SMX_ERR_UNSUPPORTED; each with a text, and the outputs keep their fill.  Zero-sized problems succeed without touching
    anything."""
    from tensor_cuda_fft_amd import _lib
    L = _lib.lib()
    B, P, Ci, Co = 2, 3, 4, 5
    x = torch.ones(B, P, Ci, dtype=torch.complex64, device=gpu)
    w = torch.ones(P, Ci, Co, dtype=torch.complex64, device=gpu)
    gy = torch.ones(B, P, Co, dtype=torch.complex64, device=gpu)
    y = torch.full((B, P, Co), 7.0, dtype=torch.complex64, device=gpu)
    gx = torch.full((B, P, Ci), 7.0, dtype=torch.complex64, device=gpu)
    gw = torch.full((P, Ci, Co), 7.0, dtype=torch.complex64, device=gpu)
    s = torch.cuda.current_stream().cuda_stream

    def fwd(xp=x.data_ptr(), wp=w.data_ptr(), yp=y.data_ptr(), b=B, p=P, ci=Ci, co=Co, mwg=0):
        return L.smx_bin_contract_forward(xp, wp, yp, b, p, ci, co, mwg, s)

    def bwd(xp=x.data_ptr(), wp=w.data_ptr(), gp=gy.data_ptr(), gxp=gx.data_ptr(), gwp=gw.data_ptr(), b=B, p=P, ci=Ci, co=Co,
            mwg=0):
        return L.smx_bin_contract_backward(xp, wp, gp, gxp, gwp, b, p, ci, co, mwg, s)
    INVALID, UNSUPPORTED = _lib.SMX_ERR_INVALID, _lib.SMX_ERR_UNSUPPORTED
    refusals = [(fwd, dict(xp=None), INVALID), (fwd, dict(wp=None), INVALID), (fwd, dict(yp=None), INVALID),
                (fwd, dict(b=-1), INVALID), (fwd, dict(p=-1), INVALID), (fwd, dict(ci=-1), INVALID), (fwd, dict(co=-1), INVALID),
                (fwd, dict(mwg=-1), INVALID), (fwd, dict(xp=x.data_ptr() + 4), INVALID), (fwd, dict(p=2 ** 31), UNSUPPORTED),
                (fwd, dict(b=2 ** 20, p=2 ** 21), UNSUPPORTED),
                (bwd, dict(gp=None), INVALID), (bwd, dict(wp=None), INVALID), (bwd, dict(xp=None), INVALID),
                (bwd, dict(b=-1), INVALID), (bwd, dict(mwg=-1), INVALID), (bwd, dict(gxp=gx.data_ptr() + 4), INVALID),
                (bwd, dict(p=2 ** 31), UNSUPPORTED)]
    for f, kw, code in refusals:
        assert f(**kw) == code, kw
        assert L.smx_last_error(), kw
    assert fwd(b=0) == 0 and fwd(p=0) == 0 and fwd(ci=0) == 0 and fwd(co=0) == 0 and fwd(b=0, xp=None, wp=None, yp=None) == 0
    assert bwd(b=0) == 0 and bwd(p=0, gp=None) == 0 and bwd(gxp=None, gwp=None) == 0
    torch.cuda.synchronize()
    for t in (y, gx, gw):
        assert bool((t == 7.0).all())
    assert bwd(xp=None, gwp=None) == 0 and bwd(wp=None, gxp=None) == 0       # the operand only the other gradient needs
    assert fwd() == 0
    torch.cuda.synchronize()
    assert bool((y == Ci).all()) and bool((gx == Co).all()) and bool((gw == B).all())


def _conv_check(name, got, leaves, x, w, want64, seed):
    """forward and both gradients of a convolution against the float64 definition"""
    assert got.dtype == torch.float32 and got.shape == want64.shape
    assert _err(name + " y", got, want64.detach(), TOL_ACT) <= TOL_ACT
    g = torch.randn(want64.shape, generator=torch.Generator().manual_seed(seed))
    gx, gw = torch.autograd.grad(got, leaves, g.to(got.device))
    dx, dw = torch.autograd.grad(want64, (x, w), g.double())
    assert _err(name + " grad_x", gx, dx, TOL_ACT) <= TOL_ACT
    assert _err(name + " grad_w", gw, dw, TOL_PARAM) <= TOL_PARAM


@pytest.mark.parametrize("case", oc.CONV1D + [oc.CONV1D_FOURSTEP], ids=lambda c: "x".join(map(str, c)))
def test_conv1d_forward_and_gradients(gpu, case):
    import tensor_cuda_fft_amd as pkg
    x, w = oc.conv1d_inputs(case)
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    xd, wd = x.to(gpu).requires_grad_(), w.to(gpu).requires_grad_()
    y = pkg.OptimizedFrequencyOps.fast_frequency_conv1d(xd, wd, stride=case[6], padding=case[5])
    _conv_check(f"conv1d {case}", y, (xd, wd), x64, w64, oc.conv1d_def(x64, w64, case[6], case[5]), 5)


@pytest.mark.parametrize("case", oc.CONV2D, ids=lambda c: "x".join(map(str, c[:7])))
def test_conv2d_forward_and_gradients(gpu, case):
    import tensor_cuda_fft_amd as pkg
    x, w = oc.conv2d_inputs(case)
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    xd, wd = x.to(gpu).requires_grad_(), w.to(gpu).requires_grad_()
    y = pkg.OptimizedFrequencyOps.fast_frequency_conv2d(xd, wd, stride=case[8], padding=case[7])
    _conv_check(f"conv2d {case[:7]}", y, (xd, wd), x64, w64, oc.conv2d_def(x64, w64, case[8], case[7]), 6)


def test_the_convolutions_run_the_native_contraction(gpu, monkeypatch):
    """the K > 64 and the large-kernel 2-D branches go through smx_bin_contract_forward; K = 64 and 7 x 7 equal
    F.conv1d / F.conv2d, the other branch"""
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import _lib
    O = pkg.OptimizedFrequencyOps
    calls = []
    real = _lib.lib().smx_bin_contract_forward
    monkeypatch.setattr(_lib.lib(), "smx_bin_contract_forward", lambda *a: (calls.append(a[3:7]), real(*a))[1], raising=False)
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(2, 3, 100, generator=g).to(gpu), torch.randn(4, 3, 64, generator=g).to(gpu)
    assert torch.equal(O.fast_frequency_conv1d(x, w, 2, 3), torch.nn.functional.conv1d(x, w, stride=2, padding=3))
    x2, w2 = torch.randn(2, 3, 12, 13, generator=g).to(gpu), torch.randn(4, 3, 7, 7, generator=g).to(gpu)
    assert torch.equal(O.fast_frequency_conv2d(x2, w2, (2, 1), 1), torch.nn.functional.conv2d(x2, w2, stride=(2, 1), padding=1))
    assert calls == []
    O.fast_frequency_conv1d(x, torch.randn(4, 3, 65, generator=g).to(gpu))
    O.fast_frequency_conv2d(x2, torch.randn(4, 3, 8, 2, generator=g).to(gpu))
    assert calls == [(2, 129, 3, 4), (2, 17 * 16, 3, 4)]


def test_topk_and_sparse_fft_equal_the_reference_exactly(gpu):
    import tensor_cuda_fft_amd as pkg
    O = pkg.OptimizedFrequencyOps
    rec = load_golden("O20_optops_members")
    data, k = torch.from_numpy(rec["topk.data"]), int(rec["topk.k"])
    oc.assert_separated(data, k)
    v, i = O.fast_topk_sparse(data.to(gpu), k)
    assert i.dtype == torch.int64 and v.shape == i.shape == (k,)
    assert np.array_equal(i.cpu().numpy(), rec["topk.indices"]) and np.array_equal(v.cpu().numpy(), rec["topk.values"])
    big = oc.separated_spectrum((70, 130), 1000, seed=9)              # more than one tile of the radix select
    oc.assert_separated(big, 1000)
    v, i = O.fast_topk_sparse(big.to(gpu), 1000)
    wi = torch.topk(torch.abs(big.flatten()), 1000).indices
    assert torch.equal(i.cpu(), wi) and torch.equal(v.cpu(), big.flatten()[wi])
    sp = torch.from_numpy(rec["sfft.x"])
    oc.assert_separated(torch.fft.fftn(sp), rec["sfft.coeffs"].size)
    c, idx = O.optimized_sparse_fft(sp.to(gpu), float(rec["sfft.sparsity"]))
    assert np.array_equal(idx.cpu().numpy(), rec["sfft.indices"])
    assert _err("sparse_fft coeffs", c, torch.fft.fftn(sp.to(torch.complex128)).flatten()[torch.from_numpy(rec["sfft.indices"])],
                TOL_ACT) <= TOL_ACT
    back = O.optimized_sparse_ifft(c, idx, (8, 12), device=str(gpu))
    full = torch.zeros(96, dtype=torch.complex128)
    full[torch.from_numpy(rec["sfft.indices"])] = torch.from_numpy(rec["sfft.coeffs"]).to(torch.complex128)
    assert back.dtype == torch.float32
    assert _err("sparse_ifft", back, torch.fft.ifftn(full.reshape(8, 12)).real, TOL_ACT) <= TOL_ACT


def test_matmul_on_both_branches(gpu):
    import tensor_cuda_fft_amd as pkg
    O = pkg.OptimizedFrequencyOps
    rec = load_golden("O20_optops_members")
    x, wf = torch.from_numpy(rec["matmul.x"]), torch.from_numpy(rec["matmul.w_freq"])
    assert _err("matmul", O.fast_frequency_matmul(x.to(gpu), wf.to(gpu)), oc.matmul_def(x, wf), TOL_ACT) <= TOL_ACT
    # the block branch needs a weight of at least 100 MB as float32: K N = 52 * 2**19; eight blocks of 2**16 columns
    K, N, bs = 52, 1 << 19, 1 << 16
    assert K * N * 4 / 1024 ** 2 >= 100
    g = torch.Generator().manual_seed(8)
    xb = torch.randn(1, 2, K, generator=g)
    wb = oc.crandn(g, K, N)
    out = O.fast_frequency_matmul(xb.to(gpu), wb.to(gpu), block_size=bs)
    want = torch.cat([oc.matmul_def(xb, wb[:, n:n + bs]) for n in range(0, N, bs)], dim=-1)
    assert _err("matmul, block branch", out, want, TOL_ACT) <= TOL_ACT


def test_linear_forward_and_backward_against_the_golden(gpu):
    import tensor_cuda_fft_amd as pkg
    rec = load_golden("O20_optops_members")
    state = {k[len("linear.state."):]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("linear.state.")}
    lin = pkg.ProductionFrequencyLinear(48, 10, sparsity=0.25)
    lin.load_state_dict(state, strict=True)
    lin.to(gpu)
    x, g = torch.from_numpy(rec["linear.x"]), torch.from_numpy(rec["linear.g"])
    w64 = state["weight_freq"].to(torch.complex128).requires_grad_()
    b64 = state["bias"].double().requires_grad_()
    want = torch.nn.functional.linear(x.double(), torch.fft.ifft(w64, dim=-1).real, b64)
    want.backward(g.double())
    y = lin(x.to(gpu))
    y.backward(g.to(gpu))
    assert _err("linear y", y, want.detach(), TOL_ACT) <= TOL_ACT
    assert _err("linear grad weight_freq", lin.weight_freq.grad, w64.grad, TOL_PARAM) <= TOL_PARAM
    assert _err("linear grad bias", lin.bias.grad, b64.grad, TOL_PARAM) <= TOL_PARAM
    assert rel_err(y.detach().cpu().numpy(), rec["linear.out"]) <= TOL_ACT


def test_production_ops_on_the_device(gpu):
    import tensor_cuda_fft_amd as pkg
    rec = load_golden("O20_optops_members")
    P = pkg.ProductionFrequencyOps
    t = torch.from_numpy(rec["compress.x"])
    comp = P.compress_tensor(t.to(gpu), sparsity=float(rec["compress.sparsity"]))
    assert comp.use_cuda and np.array_equal(comp.indices.cpu().numpy(), rec["compress.indices"].astype(np.int64))
    bx = torch.from_numpy(rec["bsm.x"])
    out = P.block_streaming_matmul(bx.to(gpu), comp, block_size=int(rec["bsm.block_size"]))
    assert rel_err(out.cpu().numpy(), rec["bsm.out"]) <= TOL_ACT
    o = pkg.OptimizedSparseSpectralTensor(data=t.to(gpu), sparsity=float(rec["compress.sparsity"]))
    first = o.to_spatial()
    assert o.to_spatial() is first and rel_err(first.cpu().numpy(), rec["osst.to_spatial"]) <= TOL_ACT


def _bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


def test_two_runs_and_a_graph_replay_are_bitwise_equal(gpu):
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import functional as fn
    x, w, gy = (t.to(gpu) for t in _operands((9, 70, 17, 33), seed=21))
    x.requires_grad_(), w.requires_grad_()
    cx, cw = (t.to(gpu) for t in oc.conv1d_inputs(oc.CONV1D[1]))

    def step():
        y = fn.bin_contract(x, w)
        gx, gw = torch.autograd.grad(y, (x, w), gy)
        return y.detach(), gx, gw, pkg.OptimizedFrequencyOps.fast_frequency_conv1d(cx, cw, 2, 4)
    first = [t.clone() for t in step()]                      # (eager once before the capture: INTEGRATION.md)
    for a, b in zip(step(), first):
        assert torch.equal(_bits(a), _bits(b))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, first):
        assert torch.equal(_bits(a), _bits(b))
