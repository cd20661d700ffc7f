"""SpectralEMA / ChunkLM on the GPU: the one-launch scan (csrc/smx_ema.hip) against the reference's golden vectors and
against an fp64 evaluation of the reference's op sequence (tests/ema_common.py)."""
import math

import numpy as np
import pytest
import torch

import ema_common as ec
from conftest import TOL_ACT, TOL_PARAM, load_golden, rel_err

pytestmark = pytest.mark.gpu

SCANS = ("S01_ema_aligned_3x64x9", "S02_ema_polar_2x37x33", "S03_ema_init_2x5x130", "S04_ema_update_2x1x9")
HEADS = ("C01_chunklm_2x64", "C02_chunklm_2x100_L12")
KEYS = ("state", "grad_chunks", "grad_init", "grad_rho_logit", "grad_theta_raw")


def tol(key):
    return TOL_ACT if key in ("state", "grad_chunks", "grad_init", "y") else TOL_PARAM


def _run(scan, chunks, rl, tr, init, g):
    """forward + backward of `scan(chunks, rl, tr, init)`; every result as numpy (None where there is no gradient)."""
    y = scan(chunks, rl, tr, init)
    y.backward(g)
    out = {"state": y.detach(), "grad_chunks": chunks.grad, "grad_rho_logit": rl.grad, "grad_theta_raw": tr.grad,
           "grad_init": None if init is None else init.grad}
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _inputs(z, dev):
    return (ec.t(z["chunks"], dev, grad=True), ec.t(z["sd.rho_logit"], dev, grad=True),
            ec.t(z["sd.theta_raw"], dev, grad=True), ec.t(z["init"], dev, grad=True) if "init" in z else None,
            ec.t(z["g"], dev))


def _check(got, ref, keys=KEYS):
    for k in keys:
        if ref.get(k) is not None:
            e = rel_err(got[k], ref[k])
            print(f"{k}: {e:.2e}")
            assert e <= tol(k), (k, e)


@pytest.mark.parametrize("name", SCANS)
@pytest.mark.parametrize("through", ["module", "functional"])
def test_scan_matches_the_reference(gpu, name, through):
    import tensor_cuda_fft_amd as pkg
    z = load_golden(name)
    mode = str(z["mode"])
    chunks, rl, tr, init, g = _inputs(z, gpu)
    if through == "module":
        m = pkg.SpectralEMA(pkg.EMAConfig(n_freqs=chunks.shape[2], mode=mode)).to(gpu)
        m.load_state_dict({"rho_logit": rl.detach(), "theta_raw": tr.detach()})
        got = _run(lambda c, *_: m.scan(c, init), chunks, m.rho_logit, m.theta_raw, init, g)
    else:
        got = _run(lambda c, r, t_, i: pkg.ema_scan(c, r, t_, mode, i), chunks, rl, tr, init, g)
    _check(got, z)
    if mode == "polar":
        assert got["grad_theta_raw"] is None


def _fp64(chunks, rl, tr, mode, init, g):
    c = chunks.detach().cpu().to(torch.complex128).requires_grad_(True)
    r = rl.detach().cpu().double().requires_grad_(True)
    t_ = tr.detach().cpu().double().requires_grad_(True)
    i = None if init is None else init.detach().cpu().to(torch.complex128).requires_grad_(True)
    return _run(lambda *a: ec.scan_ref(a[0], a[1], a[2], mode, a[3]), c, r, t_, i, g.cpu().to(torch.complex128))


@pytest.mark.parametrize("mode,B,S,F,with_init", [("aligned", 3, 64, 9, False), ("polar", 2, 37, 33, False),
                                                  ("aligned", 2, 5, 130, True), ("aligned", 2, 1, 9, True),
                                                  ("polar", 2, 5, 130, True)])
def test_scan_matches_an_fp64_evaluation_of_the_reference_sequence(gpu, mode, B, S, F, with_init):
    import tensor_cuda_fft_amd as pkg
    gen = torch.Generator().manual_seed(4321)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    chunks = torch.complex(rnd(B, S, F), rnd(B, S, F))
    if S > 2:
        chunks[B - 1, S // 2] = 0
        chunks[0, 0, F // 2] = 0
    chunks = chunks.to(gpu).requires_grad_(True)
    rl = (2.0 + rnd(F)).to(gpu).requires_grad_(True)
    tr = (0.5 * rnd(F)).to(gpu).requires_grad_(True)
    init = torch.complex(rnd(B, F), rnd(B, F)).to(gpu).requires_grad_(True) if with_init else None
    g = torch.complex(rnd(B, F), rnd(B, F)).to(gpu)
    got = _run(lambda c, r, t_, i: pkg.ema_scan(c, r, t_, mode, i), chunks, rl, tr, init, g)
    _check(got, _fp64(chunks, rl, tr, mode, init, g))


@pytest.mark.parametrize("mode", ["aligned", "polar"])
def test_grad_init_at_a_zero_state(gpu, mode):
    """At a state that is exactly zero the reference's autograd takes angle's gradient as 0 and hands conj(a rot) G to
    the state (aligned; rot = u(X)); |H|'s gradient at 0 is 0 (polar)."""
    import tensor_cuda_fft_amd as pkg
    gen = torch.Generator().manual_seed(7)
    B, F = 3, 9
    rnd = lambda *s: torch.randn(*s, generator=gen)
    x = torch.complex(rnd(B, 1, F), rnd(B, 1, F))
    x[1, 0, 4] = 0                                           # rot = 1 there
    rl, tr = 2.0 + rnd(F), 0.5 * rnd(F)
    g = torch.complex(rnd(B, F), rnd(B, F))
    init = torch.zeros(B, F, dtype=torch.complex64, device=gpu, requires_grad=True)
    pkg.ema_scan(x.to(gpu), rl.to(gpu), tr.to(gpu), mode, init).backward(g.to(gpu))
    if mode == "polar":
        assert not init.grad.any()
        return
    a = (torch.sigmoid(rl.double()) * torch.exp(1j * math.pi * torch.tanh(tr.double())))[None]
    xd = x[:, 0].to(torch.complex128)
    rot = torch.where(xd == 0, torch.ones_like(xd), xd / xd.abs().clamp_min(1e-300))
    want = torch.conj(a * rot) * g.to(torch.complex128)
    assert rel_err(init.grad.cpu().numpy(), want.numpy()) <= TOL_ACT


def test_update_is_a_scan_of_one_step_bit_for_bit(gpu):
    import tensor_cuda_fft_amd as pkg
    z = load_golden("S04_ema_update_2x1x9")
    m = pkg.SpectralEMA(pkg.EMAConfig(n_freqs=9)).to(gpu)
    m.load_state_dict({"rho_logit": ec.t(z["sd.rho_logit"]), "theta_raw": ec.t(z["sd.theta_raw"])})
    state, x = ec.t(z["init"], gpu), ec.t(z["chunks"], gpu)[:, 0]
    with torch.no_grad():
        a = m.update(state, x)
        b = m.scan(x[:, None], state)
    assert torch.equal(a, b)
    assert rel_err(a.cpu().numpy(), z["state"]) <= TOL_ACT


def _head(z, dev):
    import tensor_cuda_fft_amd as pkg
    lm = pkg.ChunkLM(ec.StubBackbone(8), int(z["chunk"]), use_ema=True, ema_chunk_len=int(z["L"]), ema_mode=str(z["mode"]))
    lm.load_state_dict({k[3:]: ec.t(v) for k, v in z.items() if k.startswith("sd.")})
    return lm.to(dev)


@pytest.mark.parametrize("name", HEADS)
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_chunk_head_matches_the_reference(gpu, name, dtype):
    z = load_golden(name)
    lm = _head(z, gpu)
    y = lm(ec.t(z["x"]).to(dtype).to(gpu))
    y.backward(ec.t(z["g"], gpu))
    e = rel_err(y.detach().cpu().numpy(), z["y"])
    print(f"y: {e:.2e}")
    assert e <= TOL_ACT
    for k, p in lm.named_parameters():
        e = rel_err(p.grad.cpu().numpy(), z["grad." + k])
        print(f"grad.{k}: {e:.2e}")
        assert e <= TOL_PARAM, (k, e)


@pytest.mark.parametrize("name", HEADS)
def test_chunk_head_matches_an_fp64_evaluation(gpu, name):
    z = load_golden(name)
    lm = _head(z, gpu)
    gen = torch.Generator().manual_seed(99)
    x = ec.conditioned_bytes(gen, 2, z["x"].shape[1], int(z["L"]))           # fresh bytes, same shape
    g = torch.randn(z["g"].shape, generator=gen)
    y = lm(x.to(gpu))
    y.backward(g.to(gpu))
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in lm.state_dict().items()}
    y64 = ec.chunklm_ref(sd, x, int(z["L"]), int(z["chunk"]), str(z["mode"]))
    y64.backward(g.double())
    assert rel_err(y.detach().cpu().numpy(), y64.detach().numpy()) <= TOL_ACT
    for k, p in lm.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), sd[k].grad.numpy()) <= TOL_PARAM, k


@pytest.mark.parametrize("mode", ["aligned", "polar"])
@pytest.mark.parametrize("B,T,L", [(2, 64, 16), (3, 100, 12), (2, 130, 64), (2, 23, 7), (65, 6, 2)])
def test_token_front_end_equals_the_scan_of_the_fp64_spectra(gpu, mode, B, T, L):
    import tensor_cuda_fft_amd as pkg
    gen = torch.Generator().manual_seed(5)
    F = L // 2 + 1
    x = ec.conditioned_bytes(gen, B, T, L)
    rl = (2.0 + torch.randn(F, generator=gen)).to(gpu)
    tr = (0.5 * torch.randn(F, generator=gen)).to(gpu)
    chunks = ec.byte_chunks(x, L).to(torch.complex64).to(gpu)               # formed in fp64, rounded once
    g = torch.complex(torch.randn(B, F, generator=gen), torch.randn(B, F, generator=gen)).to(gpu)
    res = []
    for scan in (lambda r, t_: pkg.ema_scan(chunks, r, t_, mode),
                 lambda r, t_: pkg.ema_scan_tokens(x.to(gpu), L, r, t_, mode),
                 lambda r, t_: pkg.ema_scan_tokens(x.to(torch.uint8).to(gpu), L, r, t_, mode),
                 lambda r, t_: pkg.ema_scan_tokens(torch.cat([x, x], 1).to(gpu)[:, :T], L, r, t_, mode)):   # a row stride
        r, t_ = rl.clone().requires_grad_(True), tr.clone().requires_grad_(True)
        y = scan(r, t_)
        y.backward(g)
        res.append((y.detach().cpu().numpy(), r.grad.cpu().numpy(), None if t_.grad is None else t_.grad.cpu().numpy()))
    ref = res[0]
    for got in res[1:]:
        assert rel_err(got[0], ref[0]) <= TOL_ACT
        assert rel_err(got[1], ref[1]) <= TOL_PARAM
        assert (got[2] is None) == (mode == "polar")
        if mode == "aligned":
            assert rel_err(got[2], ref[2]) <= TOL_PARAM
    for a, b in zip(res[1], res[2]):                                          # int64 and uint8 tokens: the same bits
        assert a is None and b is None or np.array_equal(a, b)


def test_exactly_cancelling_chunks_take_unit_phase(gpu):
    """The DC and Nyquist bins are integer sums and a run of equal bytes cancels exactly in every bin f > 0: those
    bins are exactly zero and take u = 1 (the reference follows the sign of its FFT's rounding noise there)."""
    import tensor_cuda_fft_amd as pkg
    L, F = 16, 9
    x = torch.full((2, 2 * L), 200, dtype=torch.int64)
    x[1, L:] = torch.tensor([255, 0] * 8)                    # second chunk: the DC bin of (2 b - 255) cancels exactly
    rl, tr = torch.full((F,), 2.0, device=gpu), torch.zeros(F, device=gpu)
    y = pkg.ema_scan_tokens(x.to(gpu), L, rl, tr, "polar").cpu()
    rho = 1 / (1 + math.exp(-2.0))
    dc = L * (200 / 127.5 - 1)
    assert torch.count_nonzero(y[0, 1:]) == 0 and y[0].imag.abs().max() == 0
    assert abs(float(y[0, 0].real) - (rho * (1 - rho) * dc + (1 - rho) * dc)) <= 1e-5 * dc
    # row 1: the state (1 - rho) dc meets a DC bin that is exactly zero -> rho |H| u with u = 1: real, positive
    assert float(y[1, 0].imag) == 0 and abs(float(y[1, 0].real) - rho * (1 - rho) * dc) <= 1e-5 * dc


def test_two_runs_are_bitwise_identical_and_a_strided_view_changes_nothing(gpu):
    import tensor_cuda_fft_amd as pkg
    z = load_golden("S03_ema_init_2x5x130")
    runs = []
    for k in range(3):
        chunks, rl, tr, init, g = _inputs(z, gpu)
        if k == 2:                                           # every other bin of a twice-as-wide buffer
            wide = torch.zeros(2, 5, 260, dtype=torch.complex64, device=gpu)
            wide[:, :, ::2] = chunks.detach()
            wide.requires_grad_(True)
            view = wide[:, :, ::2]
            assert not view.is_contiguous()
            y = pkg.ema_scan(view, rl, tr, "aligned", init)
            y.backward(g)
            runs.append([y.detach(), wide.grad[:, :, ::2], rl.grad, tr.grad, init.grad])
            assert not wide.grad[:, :, 1::2].any()
        else:
            y = pkg.ema_scan(chunks, rl, tr, "aligned", init)
            y.backward(g)
            runs.append([y.detach(), chunks.grad, rl.grad, tr.grad, init.grad])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_no_grad_forward_saves_nothing_and_empty_scan_copies_init(gpu):
    import tensor_cuda_fft_amd as pkg
    rl, tr = torch.zeros(9, device=gpu, requires_grad=True), torch.zeros(9, device=gpu, requires_grad=True)
    init = torch.randn(2, 9, dtype=torch.complex64, device=gpu)
    with torch.no_grad():
        y = pkg.ema_scan(torch.randn(2, 4, 9, dtype=torch.complex64, device=gpu), rl, tr, "aligned", init)
    assert y.grad_fn is None and not y.requires_grad
    empty = torch.empty(2, 0, 9, dtype=torch.complex64, device=gpu)
    assert torch.equal(pkg.ema_scan(empty, rl, tr, "aligned", init), init)
    assert not pkg.ema_scan(empty, rl, tr, "polar").any()


def test_captured_step_sees_an_in_place_parameter_update(gpu):
    """rho_logit / theta_raw are read from device memory inside the kernels: a captured forward+backward replayed after
    an in-place change computes with the new values."""
    import tensor_cuda_fft_amd as pkg
    z = load_golden("S01_ema_aligned_3x64x9")
    chunks, rl, tr, _, g = _inputs(z, gpu)

    def step():
        y = pkg.ema_scan(chunks, rl, tr, "aligned")
        return (y,) + torch.autograd.grad(y, (chunks, rl, tr), g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, step()):
        assert torch.equal(a, b)
    with torch.no_grad():
        rl.sub_(1.0)
        tr.add_(0.25)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = step()
    assert not torch.equal(replayed[0], ec.t(z["state"], gpu))
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)


def test_short_window_leaves_the_head_alone(gpu):
    import tensor_cuda_fft_amd as pkg
    torch.manual_seed(0)
    lm = pkg.ChunkLM(ec.StubBackbone(8), 2, use_ema=True, ema_chunk_len=16).to(gpu)
    x = torch.randint(0, 256, (2, 15), device=gpu)
    plain = lm.head(lm.backbone.forward_hidden(x)[:, -1]).view(2, 2, 256)
    assert torch.equal(lm(x), plain)
