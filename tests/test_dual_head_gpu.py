"""The dual head on the GPU: k_xent_* against fp64 autograd of F.cross_entropy on every (VEC, CH) instance of the register
rows and every misalignment and tail of the streaming rows, rows read in place through a stride, the edge semantics of
include/smx.h (-inf, +inf, all rows ignored, targets out of range), bitwise reproducibility, the module against the
reference's fixture (K21), the 50257-wide model, one training step over a FixedSpectralLM, and the step in a graph."""
import numpy as np
import pytest
import torch

import dual_common as dc
import heads_common as hc
from conftest import TOL_ACT, TOL_PARAM, load_golden, rel_err

pytestmark = pytest.mark.gpu

# (VEC, CH) of the register rows by width: 1 2 6 <1,1>, 64 256 <4,1>, 130 255 <1,4>, 257 1022 <1,16>, 260 512 <4,2>,
# 1024 <4,4>, 1028 <4,8>, 2052 4096 <4,16>
REG_V = [1, 2, 6, 64, 130, 255, 256, 257, 260, 512, 1022, 1024, 1028, 2052, 4096]
STREAM_V = [1025, 1026, 1027, 4097, 4099, 4100, 5000, 8193, 50257]         # every V mod 4: every row misalignment and tail
REG_ROWS = [1, 37, 111]                  # 111 rows: a ragged last block of ROW_WAVES = 4
STREAM_ROWS = [1, 3, 5]
REDUCTIONS = ["mean", "sum", "none"]
REG_WALK_ROWS = 8193                     # more than LN_MAX_BLOCKS * ROW_WAVES = 8192 rows: a wave takes a second row
STREAM_WALK_ROWS = 2049                  # more than the 2048 workgroups of the streaming grid: one takes a second row
NINF = float("-inf")


def _pkg():
    import tensor_cuda_fft_amd as pkg
    return pkg


def _node(y):
    """the _CrossEntropy node within two steps of y's grad_fn (behind the reshaping views), or None"""
    todo = [y.grad_fn]
    for _ in range(3):
        for f in todo:
            if f is not None and type(f).__name__.startswith("_CrossEntropy"):
                return f
        todo = [g for f in todo if f is not None for g, _ in f.next_functions]
    return None


def _targets(gen, R, V, ignore_index, ignored):
    y = gen.integers(0, V, R)
    if ignored:
        y[gen.random(R) < 0.3] = ignore_index
        y[0] = ignore_index
    return y


def _upstream(gen, R, reduction, dev):
    """upstream gradient, not 1: (R) for "none", a 0-d tensor otherwise"""
    g = torch.from_numpy(gen.standard_normal(R).astype(np.float32)).to(dev) + 1.5
    return g if reduction == "none" else g[0].clone()


def _ref64(x, y, ignore_index, reduction, g):
    """loss, gradient and lse (0 on ignored rows) by fp64 autograd of F.cross_entropy"""
    x64 = x.detach().double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x64, y, ignore_index=ignore_index, reduction=reduction)
    loss.backward(g.double())
    lse = torch.logsumexp(x64.detach(), -1)
    lse = torch.where(y == ignore_index, torch.zeros_like(lse), lse)
    return loss.detach(), x64.grad, lse


def _close(a, ref, what):
    a, ref = a.detach().cpu().numpy(), ref.detach().cpu().numpy()
    assert np.isfinite(ref).all(), what
    e = rel_err(a, ref)
    assert e <= TOL_ACT, (what, e)


def _check(x, y, ignore_index, reduction, g, what):
    """native forward + backward of `x` (a leaf, any layout) against the fp64 reference; returns (loss, grad)"""
    pkg = _pkg()
    x.grad = None
    loss = pkg.cross_entropy(x, y, ignore_index=ignore_index, reduction=reduction)
    node = _node(loss)
    assert node is not None, what                                       # the native path ran
    # the saved (max, log-sum) pairs, read before the backward frees them: their sum is the log-sum-exp
    lse = node.saved_tensors[2][:2 * y.numel()].view(-1, 2).double().sum(-1)
    loss.backward(g)
    ref_loss, ref_grad, ref_lse = _ref64(x, y, ignore_index, reduction, g)
    _close(loss, ref_loss, (what, "loss"))
    _close(lse, ref_lse, (what, "lse"))
    _close(x.grad, ref_grad, (what, "grad"))
    live = (y != ignore_index)
    assert not x.grad[~live].any(), what                                # ignored rows: exact zeros
    if reduction == "none":
        assert not loss.detach()[~live].any(), what
    return loss.detach(), x.grad


def _sweep(gpu, V, rows, seed):
    gen = np.random.default_rng(seed + V)
    for R in rows:
        x = hc.t((3.0 * gen.standard_normal((R, V))).astype(np.float32)).to(gpu).requires_grad_(True)
        for reduction in REDUCTIONS:
            for ignore_index, ignored in ((-100, False), (0, True)):
                y = hc.t(_targets(gen, R, V, ignore_index, ignored)).to(gpu)
                if reduction == "mean" and bool((y == ignore_index).all()):
                    continue                                            # 0 / 0: test_infinite_rows_..._all_rows_ignored
                _check(x, y, ignore_index, reduction, _upstream(gen, R, reduction, gpu), (V, R, reduction, ignored))


@pytest.mark.parametrize("V", REG_V)
def test_register_rows_match_fp64_on_every_instance(gpu, V):
    _sweep(gpu, V, REG_ROWS, 100)


@pytest.mark.parametrize("V", STREAM_V)
def test_streaming_rows_match_fp64_on_every_misalignment(gpu, V):
    _sweep(gpu, V, STREAM_ROWS, 200)


@pytest.mark.parametrize("V,R", [(6, REG_WALK_ROWS), (1025, STREAM_WALK_ROWS)])
def test_a_wave_or_workgroup_walks_to_a_second_row(gpu, V, R):
    gen = np.random.default_rng(V)
    x = hc.t((3.0 * gen.standard_normal((R, V))).astype(np.float32)).to(gpu).requires_grad_(True)
    for reduction in REDUCTIONS:
        y = hc.t(_targets(gen, R, V, 0, True)).to(gpu)
        _check(x, y, 0, reduction, _upstream(gen, R, reduction, gpu), (V, R, reduction))


# ---- rows read in place --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,width,off", [(256, 272, 0),      # aligned base, aligned stride: Vec<4> in place
                                         (256, 272, 4),      # aligned stride, base 16 bytes in: still Vec<4>
                                         (256, 272, 3),      # misaligned base: the scalar instance
                                         (256, 263, 0),      # V % 4 == 0, row_stride % 4 != 0: the scalar instance
                                         (2048, 2051, 1),    # the same beyond the scalar instances: streaming rows
                                         (4099, 4200, 0), (4099, 4201, 2), (1027, 1030, 3), (6, 9, 1)])
def test_a_last_dimension_slice_is_read_in_place(gpu, V, width, off):
    pkg = _pkg()
    gen = np.random.default_rng(width + off)
    R = 7
    wide = hc.t((3.0 * gen.standard_normal((R, width))).astype(np.float32)).to(gpu)
    wide[:, :off] = float("nan")
    wide[:, off + V:] = float("nan")                                     # nothing outside the slice may be read
    leaf = wide.clone().requires_grad_(True)
    for reduction in REDUCTIONS:
        y = hc.t(_targets(gen, R, V, 0, True)).to(gpu)
        g = _upstream(gen, R, reduction, gpu)
        x = leaf[:, off:off + V]
        loss = pkg.cross_entropy(x, y, ignore_index=0, reduction=reduction)
        node = _node(loss)
        assert node is not None
        saved = node.saved_tensors[0]
        assert saved.data_ptr() == x.data_ptr() and saved.stride(0) == width          # no copy was made
        leaf.grad = None
        loss.backward(g)
        ref_loss, ref_grad, _ = _ref64(x.detach().contiguous(), y, 0, reduction, g)
        _close(loss, ref_loss, (V, width, off, reduction, "loss"))
        _close(leaf.grad[:, off:off + V], ref_grad, (V, width, off, reduction, "grad"))
        assert not leaf.grad[:, :off].any() and not leaf.grad[:, off + V:].any()


def test_a_view_that_is_not_dense_in_its_last_dimension_is_copied(gpu):
    pkg = _pkg()
    gen = np.random.default_rng(9)
    base = hc.t((3.0 * gen.standard_normal((260, 5, 3))).astype(np.float32)).to(gpu).requires_grad_(True)
    y = hc.t(gen.integers(0, 260, (5, 3))).to(gpu)
    x = base.permute(1, 2, 0)                                            # (5, 3, 260), the last dimension strided
    loss = pkg.cross_entropy(x, y)
    node = _node(loss)
    assert node is not None and node.saved_tensors[0].is_contiguous()
    loss.backward()
    ref_loss, ref_grad, _ = _ref64(x.detach().reshape(-1, 260), y.reshape(-1), -100, "mean", torch.ones((), device=gpu))
    _close(loss, ref_loss, "loss")
    _close(base.grad.permute(1, 2, 0).reshape(-1, 260), ref_grad, "grad")
    rows = base.detach()[:, 0, :].t()[:, ::2]                            # (3, 130): rows that share no single dense layout
    rows = rows.clone().t().contiguous().t().requires_grad_(True)        # (3, 130) with strides (1, 3): copied as well
    assert rows.stride() == (1, 3)
    _check(rows, hc.t(gen.integers(0, 130, 3)).to(gpu), -100, "sum", torch.ones((), device=gpu), "column-major")


def test_rows_more_than_two_gib_apart(gpu):
    """Two rows 2^32 + 256 bytes apart in one uninitialised allocation: the row offset is formed in 64 bits.  (Element
    offsets beyond 2^31 inside one row would need more than 8 GB and are not tested.)"""
    if torch.cuda.mem_get_info()[0] < 6e9:
        pytest.skip("less than 6 GB of device memory free")
    pkg = _pkg()
    gen = np.random.default_rng(31)
    stride = 2 ** 30 + 64
    for V in (4099, 256):
        base = torch.empty(stride + V, dtype=torch.float32, device=gpu)
        x = base.as_strided((2, V), (stride, 1))
        vals = hc.t((3.0 * gen.standard_normal((2, V))).astype(np.float32)).to(gpu)
        x.copy_(vals)
        x.requires_grad_(True)
        y = hc.t(gen.integers(1, V, 2)).to(gpu)
        loss = pkg.cross_entropy(x, y, ignore_index=0, reduction="none")
        node = _node(loss)
        assert node is not None and node.saved_tensors[0].stride(0) == stride
        g = hc.t(np.array([0.5, -2.0], np.float32)).to(gpu)
        (grad,) = torch.autograd.grad(loss, x, g)
        ref_loss, ref_grad, _ = _ref64(vals, y, 0, "none", g)
        _close(loss, ref_loss, (V, "loss"))
        _close(grad, ref_grad, (V, "grad"))
        del base, x, loss, node, grad
        torch.cuda.empty_cache()


# ---- edge semantics ------------------------------------------------------------------------------------------------------

def _head_of(x, r):
    """elements of row r before its first 16-byte boundary (the scalar head of the streaming rows)"""
    return ((16 - (x.data_ptr() + 4 * r * x.stride(0)) % 16) % 16) // 4


def _share_masks(x, V, streaming):
    """name -> (R, V) bool: the elements one thread owns, the elements one wavefront owns (streaming rows), and
    everything but the last element"""
    R = x.shape[0]
    j = np.arange(V)
    out = {"all_but_last": np.tile(j < V - 1, (R, 1))}
    if streaming:
        chunk = np.stack([(j - _head_of(x, r)) // 4 for r in range(R)])           # 16-byte chunk of each body element
        body = np.stack([(j >= _head_of(x, r)) for r in range(R)])
        out["thread"] = body & (chunk % 256 == 5)
        out["wave"] = body & ((chunk % 256) // 64 == 1)
        out["first_stretch"] = np.tile(j < min(V - 1, 2048), (R, 1))               # every thread's first chunks
    else:
        vec = 4 if V % 4 == 0 else 1
        out["thread"] = np.tile((j // vec) % 64 == 5, (R, 1))
        out["first_stretch"] = np.tile(j < min(V - 1, 64 * vec), (R, 1))           # the whole first chunk of every lane
    return out


@pytest.mark.parametrize("V", [256, 1022, 2052, 4099, 5000])
def test_minus_infinity_entries_give_finite_losses(gpu, V):
    gen = np.random.default_rng(V)
    R = 3
    vals = (3.0 * gen.standard_normal((R, V))).astype(np.float32)
    probe = hc.t(vals).to(gpu)
    for name, mask in _share_masks(probe, V, V > 4096 or (V % 4 and V > 1024)).items():
        assert mask.any() and not mask.all(axis=1).any(), name
        v = vals.copy()
        v[mask] = NINF
        probe.copy_(hc.t(v))                                             # the same buffer: the alignment the masks assume
        x = probe.detach().requires_grad_(True)
        y = hc.t(np.array([int(np.flatnonzero(~m)[-1]) for m in mask])).to(gpu)   # a finite entry as the target
        for reduction in ("mean", "none"):
            loss, grad = _check(x, y, -100, reduction, _upstream(gen, R, reduction, gpu), (V, name, reduction))
            assert torch.isfinite(loss).all() and torch.isfinite(grad).all(), (V, name)
            assert not grad[hc.t(mask).to(gpu)].any(), (V, name)        # exp(-inf - lse) = 0 exactly


@pytest.mark.parametrize("V", [256, 130, 4099])
def test_infinite_rows_large_magnitudes_and_all_rows_ignored(gpu, V):
    pkg = _pkg()
    gen = np.random.default_rng(V + 1)
    vals = (3.0 * gen.standard_normal((4, V))).astype(np.float32)
    vals[1, V // 2] = np.inf                                             # a +inf row
    vals[2, :] = NINF                                                    # an all -inf row
    x = hc.t(vals).to(gpu).requires_grad_(True)
    y = hc.t(gen.integers(0, V, 4)).to(gpu)
    loss = pkg.cross_entropy(x, y, reduction="none")
    assert _node(loss) is not None
    ref = torch.nn.functional.cross_entropy(x.detach().double(), y, reduction="none")
    assert torch.isnan(loss[1]) and torch.isnan(loss[2]) and torch.isnan(ref[1]) and torch.isnan(ref[2])
    _close(loss[[0, 3]], ref[[0, 3]], "finite rows beside the NaN rows")
    (grad,) = torch.autograd.grad(loss.sum(), x)
    assert torch.isfinite(grad[[0, 3]]).all()
    assert torch.isnan(pkg.cross_entropy(x, y, reduction="mean"))
    # +-1e30 beside 0
    big = np.zeros((3, V), np.float32)
    big[0, ::3], big[1, ::2], big[2, 1::2] = 1e30, -1e30, 1e30
    big[2, ::2] = -1e30
    xb = hc.t(big).to(gpu).requires_grad_(True)
    for reduction in REDUCTIONS:
        _check(xb, hc.t(np.array([0, 1, 1])).to(gpu), -100, reduction, _upstream(gen, 3, reduction, gpu), (V, "1e30", reduction))
    # every row ignored: NaN mean (0 / 0), a gradient of exact zeros, never 0 * (1 / 0)
    xz = hc.t(vals[[0, 3]]).to(gpu).requires_grad_(True)
    yz = torch.full((2,), 7 % V, dtype=torch.int64, device=gpu)
    for reduction in REDUCTIONS:
        loss = pkg.cross_entropy(xz, yz, ignore_index=7 % V, reduction=reduction)
        assert _node(loss) is not None
        assert torch.isnan(loss) if reduction == "mean" else not loss.any()
        (grad,) = torch.autograd.grad(loss.sum(), xz)
        assert grad.shape == xz.shape and not grad.any() and not torch.isnan(grad).any()


def _raw(pkg, x, y, ignore_index, reduction, g, guard=float(12345.0)):
    """smx_xent_forward / _backward through the C ABI on buffers with a guard row either side of every output"""
    from tensor_cuda_fft_amd import functional as fn
    R, V = x.shape
    dev = x.device
    n_loss = R if reduction == 2 else 1
    lse = torch.full((R + 2, 2), guard, device=dev)
    loss = torch.full((n_loss + 2,), guard, device=dev)
    count = torch.full((3,), guard, device=dev)
    grad = torch.full((R + 2, V), guard, device=dev)
    ws = torch.zeros(fn._query("smx_xent_workspace_bytes", R, V), dtype=torch.uint8, device=dev)
    s = fn._stream(dev)
    fn._call(dev, "smx_xent_forward", x.data_ptr(), x.stride(0), y.data_ptr(), ignore_index, reduction,
             loss.data_ptr() + 4, lse.data_ptr() + 8, count.data_ptr() + 4, ws.data_ptr(), ws.numel(), R, V, s)
    fn._call(dev, "smx_xent_backward", g.data_ptr(), x.data_ptr(), x.stride(0), y.data_ptr(), ignore_index, reduction,
             lse.data_ptr() + 8, count.data_ptr() + 4, grad.data_ptr() + 4 * V, R, V, s)
    torch.cuda.synchronize()
    for buf in (lse, loss, count):
        assert (buf[0] == guard).all() and (buf[-1] == guard).all()
    assert (grad[0] == guard).all() and (grad[-1] == guard).all()
    assert not ws[:65536].any()                                          # the head of the workspace is not this op's
    return loss[1:-1], lse[1:-1].double().sum(-1), count[1], grad[1:-1]


@pytest.mark.parametrize("V", [256, 6, 4099, 1026])
def test_out_of_range_targets_poison_their_row_only(gpu, V):
    pkg = _pkg()
    gen = np.random.default_rng(V + 2)
    R = 9
    x = hc.t((3.0 * gen.standard_normal((R, V))).astype(np.float32)).to(gpu)
    yv = gen.integers(0, V, R)
    bad = {1: V, 4: -1, 6: 2 ** 40}
    for r, t in bad.items():
        yv[r] = t
    yv[2] = -100                                                         # ignore_index elsewhere
    y = hc.t(yv).to(gpu)
    good = np.array([r for r in range(R) if r not in bad])
    g = hc.t(gen.standard_normal(R).astype(np.float32)).to(gpu) + 1.5
    loss, lse, count, grad = _raw(pkg, x, y, -100, 2, g)
    assert float(count) == R - 1                                         # the poisoned rows count
    ref_loss, ref_grad, ref_lse = _ref64(x[good], y[good], -100, "none", g[good])
    assert torch.isnan(loss[list(bad)]).all() and torch.isnan(grad[list(bad)]).all()
    _close(loss[good], ref_loss, "loss of the other rows")
    _close(grad[good], ref_grad, "gradient of the other rows")
    _close(lse[good], ref_lse, "lse of the other rows")
    _close(lse[list(bad)], torch.logsumexp(x[list(bad)].double(), -1), "lse of the poisoned rows")
    for red, name in ((0, "mean"), (1, "sum")):
        loss, _, count, grad = _raw(pkg, x, y, -100, red, g[:1])
        assert torch.isnan(loss).all() and float(count) == R - 1
        assert torch.isnan(grad[list(bad)]).all() and torch.isfinite(grad[good]).all() and not grad[2].any()
    # through the public function: an ordinary result, no fault
    xr = x.clone().requires_grad_(True)
    out = _pkg().cross_entropy(xr, y, reduction="none")
    out.backward(g)
    assert torch.isnan(out[list(bad)]).all() and torch.isfinite(out[good]).all()
    assert torch.isnan(xr.grad[list(bad)]).all() and torch.isfinite(xr.grad[good]).all()


@pytest.mark.parametrize("V", [256, 1022, 4099])
def test_ignored_rows_are_not_read(gpu, V):
    gen = np.random.default_rng(V + 3)
    R = 11
    vals = (3.0 * gen.standard_normal((R, V))).astype(np.float32)
    y = hc.t(_targets(gen, R, V, 0, True)).to(gpu)
    dead = (y == 0)
    assert dead.any() and not dead.all()
    x = hc.t(vals).to(gpu).requires_grad_(True)
    xn = x.detach().clone()
    xn[dead] = float("nan")
    xn.requires_grad_(True)
    for reduction in REDUCTIONS:
        g = _upstream(gen, R, reduction, gpu)
        loss, grad = _check(x, y, 0, reduction, g, (V, reduction))
        loss_n = _pkg().cross_entropy(xn, y, ignore_index=0, reduction=reduction)
        (grad_n,) = torch.autograd.grad(loss_n, xn, g)
        assert torch.equal(loss_n, loss) and torch.equal(grad_n, grad)
        assert not grad_n[dead].any()


@pytest.mark.parametrize("V", [256, 4099])
def test_forward_and_backward_are_bitwise_reproducible(gpu, V):
    pkg = _pkg()
    gen = np.random.default_rng(V + 4)
    R = 4099                                                             # many block partials, a ragged last block
    x = hc.t((3.0 * gen.standard_normal((R, V))).astype(np.float32)).to(gpu).requires_grad_(True)
    y = hc.t(_targets(gen, R, V, 0, True)).to(gpu)
    for reduction in REDUCTIONS:
        g = _upstream(gen, R, reduction, gpu)
        runs = []
        for _ in range(2):
            loss = pkg.cross_entropy(x, y, ignore_index=0, reduction=reduction)
            assert _node(loss) is not None
            (grad,) = torch.autograd.grad(loss, x, g)
            runs.append((loss.detach().clone(), grad.clone()))
            torch.zeros(4096, device=gpu).sum()                          # other work on the stream in between
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- the module ----------------------------------------------------------------------------------------------------------

def test_dual_head_and_loss_match_the_reference_fixture(gpu):
    pkg = _pkg()
    z = load_golden("K21_dual_loss")
    got, (char_l, tok_l) = dc.run_k21(pkg, z, gpu)
    assert _node(char_l) is not None and _node(tok_l) is not None       # <4,1> rows and streaming rows
    dc.check_k21(got, z)


def test_token_aware_model_with_the_full_token_head(gpu):
    pkg = _pkg()
    torch.manual_seed(17)
    m = pkg.TokenAwareChunkLM(hc.StubBackbone(32), 4).to(gpu).train()
    with torch.no_grad():
        m.head.token_head.weight.normal_(0.0, 0.3)
        m.head.char_head.weight.normal_(0.0, 0.3)
    gen = np.random.default_rng(17)
    x = hc.t(gen.choice(np.array([32, 46] + list(range(97, 123))), (2, 48)).astype(np.int64)).to(gpu)
    y_char = hc.t(gen.integers(0, 256, (2, 4))).to(gpu)
    y_tok = pkg.get_token_ids_fast(x, dc.StubTokenizer())
    assert y_tok.is_cuda and torch.equal(y_tok, dc.stub_token_targets(x))
    y_tok[0, :6] = 0
    char_logits, token_logits = m(x)
    assert char_logits.shape == (2, 4, 256) and token_logits.shape == (2, 48, 50257)
    token_logits.retain_grad()
    total, char_l, tok_l = pkg.compute_dual_loss(char_logits, token_logits, y_char, y_tok)
    assert _node(char_l) is not None and _node(tok_l) is not None
    total.backward()
    h = m.backbone.last_hidden
    h64 = h.detach().double().requires_grad_(True)
    F = torch.nn.functional
    hd = m.head
    cl = F.linear(h64[:, -4:], hd.char_head.weight.detach().double(), hd.char_head.bias.detach().double())
    tl = F.linear(h64, hd.token_head.weight.detach().double(), hd.token_head.bias.detach().double())
    c64 = F.cross_entropy(cl.reshape(-1, 256), y_char.reshape(-1))
    tl.retain_grad()
    t64 = F.cross_entropy(tl.reshape(-1, 50257), y_tok.reshape(-1), ignore_index=0)
    (c64 + 0.5 * t64).backward()
    _close(char_l, c64, "char loss")
    _close(tok_l, t64, "token loss")
    _close(total, c64 + 0.5 * t64, "total")
    _close(token_logits.grad, tl.grad, "grad of the token logits")
    # behind the loss stands torch's fp32 GEMM over 50257 terms: the tolerance of a reduced gradient, as for parameters
    assert rel_err(h.grad.cpu().numpy(), h64.grad.cpu().numpy()) <= TOL_PARAM
    m.eval()
    with torch.no_grad():
        assert m(x).shape == (2, 4, 256)


def test_token_aware_model_trains_one_step_over_the_spectral_backbone(gpu):
    pkg = _pkg()
    torch.manual_seed(11)
    cfg = pkg.LMConfig(d_model=32, n_layers=1, seq_len=64, kernel_len=16)
    m = pkg.TokenAwareChunkLM(pkg.FixedSpectralLM(cfg), 4).to(gpu).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    gen = np.random.default_rng(5)
    bx = hc.t(gen.choice(np.array([32, 32, 46] + list(range(97, 123))), (4, 64)).astype(np.int64)).to(gpu)
    by = hc.t(gen.integers(97, 123, (4, 4)).astype(np.int64)).to(gpu)
    targets = dc.stub_token_targets(bx)
    assert targets.is_cuda and targets.shape == (4, 64) and int(targets.max()) < 50257

    def loss():
        logits, token_logits = m(bx)
        return pkg.compute_dual_loss(logits, token_logits, by, targets)

    first, char_l, tok_l = loss()
    assert torch.isfinite(first) and _node(char_l) is not None and _node(tok_l) is not None
    first.backward()
    gw = m.head.token_head.weight.grad
    assert gw is not None and float(gw.abs().max()) > 0
    opt.step()
    with torch.no_grad():
        assert float(loss()[0]) < float(first)


# ---- capture and fallbacks -----------------------------------------------------------------------------------------------

def test_heads_losses_and_backward_replay_from_a_graph(gpu):
    pkg = _pkg()
    torch.manual_seed(21)
    B, T, C, chunk = 3, 40, 32, 4
    head = pkg.DualHead(C, token_vocab_size=4099).to(gpu)
    gen = np.random.default_rng(21)
    sets = [(hc.t(gen.integers(0, 256, (B, chunk))).to(gpu), hc.t(gen.integers(0, 4099, (B, T))).to(gpu)) for _ in range(2)]
    sets[1][1][:, ::3] = 0
    y_char, y_tok = sets[0][0].clone(), sets[0][1].clone()
    h = torch.randn(B, T, C, device=gpu, requires_grad=True)
    leaves = [h] + list(head.parameters())

    def step():
        token_logits = head.token_head(h)
        char_logits = head.char_head(h[:, -chunk:])
        total, char_l, tok_l = pkg.compute_dual_loss(char_logits, token_logits, y_char, y_tok)
        assert _node(char_l) is not None and _node(tok_l) is not None
        return [total.detach(), char_l.detach(), tok_l.detach()] + list(torch.autograd.grad(total, leaves))

    eager = []
    for yc, yt in sets:
        y_char.copy_(yc)
        y_tok.copy_(yt)
        eager.append([v.clone() for v in step()])
    y_char.copy_(sets[0][0])
    y_tok.copy_(sets[0][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # one stream, one chain: no side streams inside
        outs = step()
    for i, (yc, yt) in enumerate(sets):
        y_char.copy_(yc)
        y_tok.copy_(yt)
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(outs, eager[i]):
            assert torch.equal(a, e)
    del graph


def test_fallbacks_are_torch_and_not_native(gpu):
    pkg = _pkg()
    F = torch.nn.functional
    torch.manual_seed(4)
    x = (3.0 * torch.randn(12, 260, device=gpu)).requires_grad_(True)
    y = torch.randint(0, 260, (12,), device=gpu)
    y[3] = 0
    xb = x.detach().bfloat16().requires_grad_(True)
    for reduction in REDUCTIONS:
        lb = pkg.cross_entropy(xb, y, ignore_index=0, reduction=reduction)                    # bf16 logits
        assert _node(lb) is None and lb.dtype == torch.bfloat16
        assert torch.equal(lb, F.cross_entropy(xb, y, ignore_index=0, reduction=reduction))
        assert _node(pkg.cross_entropy(x, y, ignore_index=0, reduction=reduction)) is not None    # fp32: native
        with torch.autocast("cuda", dtype=torch.bfloat16):
            la = pkg.cross_entropy(x, y, ignore_index=0, reduction=reduction)                  # under autocast
            ra = F.cross_entropy(x, y, ignore_index=0, reduction=reduction)
        assert _node(la) is None and torch.equal(la, ra)
    y32 = y.to(torch.int32)                                                                     # int32 targets
    try:
        ref = F.cross_entropy(x, y32, ignore_index=0)
    except (RuntimeError, TypeError) as e:                                                      # torch refuses them: so do we
        with pytest.raises(type(e)):
            pkg.cross_entropy(x, y32, ignore_index=0)
    else:
        got = pkg.cross_entropy(x, y32, ignore_index=0)
        assert _node(got) is None and torch.equal(got, ref)
    lb.sum().backward()
    assert xb.grad is not None
