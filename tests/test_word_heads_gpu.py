"""The word-structure heads on the GPU: k_word_targets against the fp64 closed form and the reference's golden vectors
over every thread-run shape, k_head_fwd / k_head_bwd against fp64 autograd of F.linear on every (VEC, CH) instance of
the row dispatch, the two models against the reference's fixtures and in one training step over a FixedSpectralLM, and
the whole step captured in a graph."""
import functools

import numpy as np
import pytest
import torch

import heads_common as hc
from conftest import TOL_ACT, TOL_PARAM, load_golden, rel_err

pytestmark = pytest.mark.gpu

T_LIST = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 4099]
LONG_T = [16385, 40000, 65536]          # 2, 3 and 4 words of 64 positions per thread (hc.thread_run: 128, 192, 256)
# (VEC, CH) of the row dispatch by width: 6 <1,1>, 8 32 128 <4,1>, 130 <1,4>, 258 510 514 <1,16>, 260 384 512 <4,2>,
# 516 <4,4>, 1028 <4,8>, 2052 <4,16>
WIDTHS = [6, 8, 32, 512, 128, 130, 258, 260, 384, 510, 514, 516, 1028, 2052]
ROWS = [1, 37, 111]                      # 111 rows: a ragged last block of ROW_WAVES = 4
WALK_ROWS = 8193                         # more than LN_MAX_BLOCKS * ROW_WAVES = 8192 rows: a wave takes a second row


def _pkg():
    import tensor_cuda_fft_amd as pkg
    return pkg


def _is_native(y):
    """y came out of the native head: a _NarrowHead node within two steps of its grad_fn (behind the reshaping views)"""
    seen, todo = [], [y.grad_fn]
    for _ in range(3):
        seen += [f for f in todo if f is not None]
        todo = [g for f in todo if f is not None for g, _ in f.next_functions]
    return any(type(f).__name__.startswith("_NarrowHead") for f in seen)


@functools.lru_cache(None)
def _cases(B, T):
    """name -> (bytes, fp64 phase, fp64 boundary), computed once and shared by the token dtypes"""
    out = {}
    for name, x in hc.patterns(B, T).items():
        out[name] = (x, hc.phase_closed_form(x), hc.boundary_closed_form(x))
    return out


def _check_targets(x_dev, ref_p, ref_b, what):
    pkg = _pkg()
    ph, bd = pkg.word_targets(x_dev)
    assert ph.is_cuda and bd.is_cuda and ph.dtype == torch.float32 and bd.dtype == torch.float32
    got_p, got_b = ph.cpu().numpy(), bd.cpu().numpy()
    assert np.array_equal(got_b, ref_b), what
    assert rel_err(got_p, ref_p) <= TOL_ACT, what
    exact = (ref_p == 0).all(-1) | ((ref_p[..., 0] == 1) & (ref_p[..., 1] == 0))      # delimiters and word starts
    assert np.array_equal(got_p[exact], ref_p[exact].astype(np.float32)), what
    only_p, none_b = pkg.word_targets(x_dev, boundary=False)
    none_p, only_b = pkg.word_targets(x_dev, phase=False)
    assert none_b is None and none_p is None and torch.equal(only_p, ph) and torch.equal(only_b, bd), what


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("T", T_LIST)
def test_targets_every_pattern(gpu, T, dtype):
    for B in (1, 3):
        for name, (x, ref_p, ref_b) in _cases(B, T).items():
            _check_targets(hc.t(x).to(dtype).to(gpu), ref_p, ref_b, (B, T, name))


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("T", LONG_T)
def test_targets_with_several_words_per_thread(gpu, T, dtype):
    cases = _cases(1, T)
    for name in ("uniform", "one_word", "run_edge_-1", "run_edge_+0", "run_edge_+1", "sets_disagree"):
        x, ref_p, ref_b = cases[name]
        _check_targets(hc.t(x).to(dtype).to(gpu), ref_p, ref_b, (T, name))


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("T", [1, 65, 1000])
def test_targets_of_strided_views(gpu, T, dtype):
    pkg = _pkg()
    x, ref_p, ref_b = _cases(3, T)["uniform"]
    wide = torch.full((3, T + 37), 32, dtype=dtype, device=gpu)
    wide[:, 5:5 + T] = hc.t(x).to(dtype).to(gpu)
    view = wide[:, 5:5 + T]                                  # a column slice: row stride T + 37, read in place
    assert not view.is_contiguous() or T == 1
    _check_targets(view, ref_p, ref_b, ("slice", T))
    two = torch.zeros((3, 2 * T), dtype=dtype, device=gpu)
    two[:, ::2] = view
    _check_targets(two[:, ::2], ref_p, ref_b, ("step 2", T))   # element stride 2: copied first


def test_targets_of_int64_values_outside_a_byte(gpu):
    for T in (7, 300):
        x = hc.wide_values(3, T)
        _check_targets(hc.t(x).to(gpu), hc.phase_closed_form(x), hc.boundary_closed_form(x), ("wide", T))


@pytest.mark.parametrize("key", ["text", "random", "edge"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
def test_targets_match_the_reference_fixture(gpu, key, dtype):
    pkg = _pkg()
    z = load_golden("K01_word_targets")
    x = hc.t(z[key + ".x"]).to(dtype).to(gpu)
    ph, bd = pkg.word_targets(x)
    assert np.array_equal(bd.cpu().numpy(), z[key + ".boundary"])
    assert rel_err(ph.cpu().numpy(), z[key + ".phase"]) <= TOL_ACT
    assert torch.equal(pkg.generate_phase_targets(x), ph) and torch.equal(pkg.get_word_boundaries(x), bd)
    _check_targets(x, hc.phase_closed_form(z[key + ".x"]), hc.boundary_closed_form(z[key + ".x"]), key)


# ---- the row head ------------------------------------------------------------------------------------------------------

def _head_inputs(gpu, R, C, O, bias):
    gen = torch.Generator().manual_seed(1000 * R + 10 * C + O)
    h = torch.randn(R, C, generator=gen)
    w = torch.randn(O, C, generator=gen) * 0.5
    b = torch.randn(O, generator=gen) if bias else None
    g = torch.randn(R, O, generator=gen) + 0.5               # a mean, so that grad_b = sum_r g is not a cancellation
    return [None if v is None else v.to(gpu) for v in (h, w, b, g)]


def _head_case(gpu, R, C, O, bias):
    pkg = _pkg()
    from tensor_cuda_fft_amd import functional as fn
    assert fn.head_supported(C, O)
    h, w, b, g = _head_inputs(gpu, R, C, O, bias)
    lv = [v.clone().requires_grad_(True) for v in (h, w) + ((b,) if bias else ())]
    y = pkg.narrow_head(lv[0], lv[1], lv[2] if bias else None)
    assert _is_native(y)                                                       # the native path, not F.linear
    grads = torch.autograd.grad(y, lv, g, retain_graph=True)
    lv64 = [v.double().clone().requires_grad_(True) for v in (h, w) + ((b,) if bias else ())]
    y64 = torch.nn.functional.linear(lv64[0], lv64[1], lv64[2] if bias else None)
    grads64 = torch.autograd.grad(y64, lv64, g.double())
    what = (R, C, O, bias)
    assert y.shape == (R, O) and rel_err(y.detach().cpu().numpy(), y64.detach().cpu().numpy()) <= TOL_ACT, what
    for i, tol in enumerate((TOL_ACT, TOL_PARAM, TOL_PARAM)[:len(lv)]):
        assert rel_err(grads[i].cpu().numpy(), grads64[i].cpu().numpy()) <= tol, (what, i)
    again = torch.autograd.grad(y, lv, g, retain_graph=True)                   # bitwise reproducible
    assert all(torch.equal(a, c) for a, c in zip(grads, again)), what
    for i in range(len(lv)):                                                   # each gradient alone
        one = [v.clone().requires_grad_(j == i) for j, v in enumerate((h, w) + ((b,) if bias else ()))]
        yi = pkg.narrow_head(one[0], one[1], one[2] if bias else None)
        assert torch.equal(yi, y)
        assert torch.equal(torch.autograd.grad(yi, [one[i]], g)[0], grads[i]), (what, i)


@pytest.mark.parametrize("O", [1, 2])
@pytest.mark.parametrize("C", WIDTHS)
def test_head_forward_and_backward_vs_fp64_linear(gpu, C, O):
    for R in ROWS:
        for bias in (True, False):
            _head_case(gpu, R, C, O, bias)


@pytest.mark.parametrize("O", [1, 2])
@pytest.mark.parametrize("C", [6, 8])
def test_head_row_walk(gpu, C, O):
    _head_case(gpu, WALK_ROWS, C, O, True)


def test_head_leading_dimensions_and_fallbacks(gpu):
    pkg = _pkg()
    from tensor_cuda_fft_amd import functional as fn
    lin = torch.nn.functional.linear
    torch.manual_seed(3)
    h = torch.randn(3, 7, 32, device=gpu, requires_grad=True)
    w, b = torch.randn(2, 32, device=gpu, requires_grad=True), torch.randn(2, device=gpu, requires_grad=True)
    y = pkg.narrow_head(h, w, b)
    assert y.shape == (3, 7, 2) and rel_err(y.detach().cpu().numpy(), lin(h, w, b).detach().cpu().numpy()) <= TOL_ACT
    assert _is_native(y)
    y.square().sum().backward()
    assert h.grad.shape == h.shape and w.grad.shape == w.shape and b.grad.shape == b.shape
    assert not fn.head_supported(1026, 2) and not fn.head_supported(32, 3)
    for hh, ww in ((torch.randn(5, 1026, device=gpu), torch.randn(2, 1026, device=gpu)),       # an unsupported width
                   (torch.randn(5, 32, device=gpu), torch.randn(3, 32, device=gpu)),           # three outputs
                   (torch.randn(5, 32, device=gpu, dtype=torch.bfloat16),
                    torch.randn(2, 32, device=gpu, dtype=torch.bfloat16))):                    # 2-byte rows
        hh.requires_grad_(True)
        yf = pkg.narrow_head(hh, ww)
        assert not _is_native(yf) and torch.equal(yf, lin(hh, ww))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ya = pkg.narrow_head(h.detach(), w.detach(), b.detach())
        assert ya.dtype == torch.bfloat16 and torch.equal(ya, lin(h.detach(), w.detach(), b.detach()))


# ---- the models ----------------------------------------------------------------------------------------------------------

MODELS = {"K11_phaseclock_2x48x32": ("PhaseClockChunkLM", "compute_phase_clock_loss", "generate_phase_targets", "phase_head"),
          "K12_segmented_2x48x32": ("SegmentedChunkLM", "compute_segmented_loss", "get_word_boundaries", "seg_head")}


@pytest.mark.parametrize("gname", sorted(MODELS))
def test_models_match_the_reference_fixture(gpu, gname):
    pkg = _pkg()
    cls, loss_fn, target_fn, head = MODELS[gname]
    z = load_golden(gname)
    m = getattr(pkg, cls)(hc.StubBackbone(int(z["d_model"])), int(z["chunk"]))
    assert sorted(m.state_dict()) == list(z["keys"])
    m.load_state_dict({k[3:]: hc.t(v) for k, v in z.items() if k.startswith("sd.")}, strict=True)
    m.to(gpu).train()
    x = hc.t(z["x"]).to(gpu)
    aux_t = getattr(pkg, target_fn)(x)
    assert aux_t.is_cuda and rel_err(aux_t.cpu().numpy(), z["aux_targets"]) <= TOL_ACT
    logits, aux = m(x)
    assert _is_native(aux)                                                                  # the native head
    total, char_l, aux_l = getattr(pkg, loss_fn)(logits, aux, hc.t(z["y_char"]).to(gpu), aux_t)
    total.backward()
    got = {"char_logits": logits, "aux": aux, "loss_total": total, "loss_char": char_l, "loss_aux": aux_l,
           "grad.hidden": m.backbone.last_hidden.grad}
    got.update({"grad." + k: p.grad for k, p in m.named_parameters() if not k.startswith("backbone.")})
    for k, v in got.items():
        tol = TOL_PARAM if k.startswith("grad.") and k != "grad.hidden" else TOL_ACT
        assert rel_err(v.detach().cpu().numpy(), z[k]) <= tol, k
    m.eval()
    with torch.no_grad():
        only = m(x)
    assert isinstance(only, torch.Tensor) and only.shape == (2, int(z["chunk"]), 256)      # eval: char logits only


@pytest.mark.parametrize("bicameral", [False, True])
def test_phase_clock_model_trains_one_step_over_the_spectral_backbone(gpu, bicameral):
    pkg = _pkg()
    torch.manual_seed(11)
    cfg = pkg.LMConfig(d_model=32, n_layers=1, seq_len=64, kernel_len=16, bicameral=bicameral)
    m = pkg.PhaseClockChunkLM(pkg.FixedSpectralLM(cfg), 4).to(gpu).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    gen = np.random.default_rng(5)
    bx = hc.t(gen.choice(np.array([32, 46, 10] + list(range(97, 123))), (4, 64)).astype(np.int64)).to(gpu)
    by = hc.t(gen.integers(97, 123, (4, 4)).astype(np.int64)).to(gpu)
    targets = pkg.generate_phase_targets(bx)
    assert targets.is_cuda and targets.shape == (4, 64, 2)

    def loss():
        logits, pv = m(bx)
        return pkg.compute_phase_clock_loss(logits, pv, by, targets)[0]

    first = loss()
    assert torch.isfinite(first)
    first.backward()
    gw = m.phase_head.head.weight.grad
    assert gw is not None and float(gw.abs().max()) > 0
    opt.step()
    with torch.no_grad():
        assert float(loss()) < float(first)
    m.eval()
    with torch.no_grad():
        assert m(bx).shape == (4, 4, 256)


# ---- capture -------------------------------------------------------------------------------------------------------------

def test_targets_heads_and_losses_replay_from_a_graph(gpu):
    pkg = _pkg()
    F = torch.nn.functional
    torch.manual_seed(21)
    B, T, C = 3, 257, 32
    xs = [hc.t(_cases(B, T)[n][0]).to(gpu) for n in ("uniform", "sets_disagree")]
    tok = xs[0].clone()
    h = torch.randn(B, T, C, device=gpu, requires_grad=True)
    w2, b2 = (0.3 * torch.randn(2, C, device=gpu)).requires_grad_(True), torch.zeros(2, device=gpu, requires_grad=True)
    w1, b1 = (0.3 * torch.randn(1, C, device=gpu)).requires_grad_(True), torch.zeros(1, device=gpu, requires_grad=True)
    leaves = [h, w2, b2, w1, b1]

    def step():
        ph, bd = pkg.word_targets(tok)
        loss = F.mse_loss(pkg.narrow_head(h, w2, b2), ph) \
            + F.binary_cross_entropy_with_logits(pkg.narrow_head(h, w1, b1).squeeze(-1), bd)
        return [loss.detach(), ph, bd] + list(torch.autograd.grad(loss, leaves))

    eager = [[v.clone() for v in step()]]
    tok.copy_(xs[1])
    eager.append([v.clone() for v in step()])
    tok.copy_(xs[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # one stream, one chain: no side streams inside
        outs = step()
    for i in range(2):
        tok.copy_(xs[i])
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(outs, eager[i]):
            assert torch.equal(a, e)
    del graph
