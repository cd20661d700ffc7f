"""EnhancedSpectralBlock and its members on the GPU (reference fft_tensor/spectral_enhancements.py:20-116, :278-333):
the fused row kernels (csrc/smx_enh.hip) against the reference's fixtures (tests/golden/E*.npz), against a float64
torch evaluation of the reference's op sequence, with the library's dropout mask, under stream capture, and as the
drop-in block of benchmark_enhanced.py's model.

Tolerances: max|delta| <= 2e-5 max|ref| for activations and input gradients, 1e-4 for parameter gradients.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, TOL_PARAM, load_golden, rel_err
from oracle import spectral_oracle as so

pytestmark = pytest.mark.gpu
TOL = 2e-5
T = torch.from_numpy


def _pkg():
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import functional
    return pkg, functional


def _load(mod, z, gpu):
    sd = {k[3:]: T(v) for k, v in z.items() if k.startswith("sd.")}
    mod.load_state_dict(sd, strict=True)
    return mod.to(gpu)


def _check_fixture(mod, z, gpu):
    x = T(z["x"]).to(gpu).requires_grad_(True)
    y = mod(x)
    y.backward(T(z["g"]).to(gpu))
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu().numpy()
    assert rel_err(c(y), z["y"]) <= TOL
    assert rel_err(c(x.grad), z["grad_x"]) <= TOL
    for name, p in mod.named_parameters():
        assert rel_err(c(p.grad), z["grad." + name]) <= TOL_PARAM, name


@pytest.mark.parametrize("name", ["E01_enh_2x256x32", "E02_enh_2x100x16", "E03_enh_1x1024x8", "E04_enh_3x40x6"])
def test_block_matches_reference_fixture(gpu, name):
    pkg, fn = _pkg()
    z = load_golden(name)
    blk = _load(pkg.EnhancedSpectralBlock(z["x"].shape[2], dropout=0.0), z, gpu)
    assert blk._fusable(T(z["x"]).to(gpu))
    _check_fixture(blk, z, gpu)


def test_rope_matches_reference_fixture(gpu):
    pkg, _ = _pkg()
    z = load_golden("E11_rope_2x300x34")
    _check_fixture(_load(pkg.RotaryFrequencyEmbedding(34), z, gpu), z, gpu)


def test_gated_unit_matches_reference_fixture(gpu):
    pkg, _ = _pkg()
    z = load_golden("E21_gsu_2x64x24")
    m = _load(pkg.GatedSpectralUnit(24), z, gpu)
    assert m._blend_native(T(z["x"]).to(gpu))
    _check_fixture(m, z, gpu)


# ---- float64 evaluation of the reference's op sequence, from the block's own parameters -------------------------------

def _ln(n, t, w=None, b=None):
    return F.layer_norm(t, t.shape[-1:], n.weight if w is None else w, n.bias if b is None else b, n.eps)


def _rope64(rotation, t):
    B, T_, D = t.shape
    pr = t.reshape(B, T_, -1, 2)
    r = torch.complex(pr[..., 0], pr[..., 1]) * rotation[:T_, :D // 2].to(torch.complex128).unsqueeze(0)
    return torch.stack([r.real, r.imag], -1).reshape(B, T_, D)


def _blend(a, v, ln):
    gate, vt = _ln(ln, a).chunk(2, dim=-1)
    gate = torch.sigmoid(gate)
    return gate * v + (1 - gate) * vt


def _block64(b, x):
    g, ms = b.gated, b.multi_scale
    x = x + _rope64(b.rope.rotation, _ln(b.norm1, x))
    x = x + so.phase_aware_port(_ln(b.norm2, x), b.phase_mixing.magnitude_filter, b.phase_mixing.phase_filter)
    h = _ln(b.norm3, x)
    x = x + _blend(g.gate_proj[0](h), g.value_proj(h), g.gate_proj[1])
    lo, mid, hi = so.multiscale_bands_port(x)
    return x + ms.fusion(torch.cat([ms.low_freq(lo), ms.mid_freq(mid), ms.high_freq(hi)], -1))


def _randomized_block(pkg, D, gpu, seed=0):
    torch.manual_seed(seed)
    blk = pkg.EnhancedSpectralBlock(D, dropout=0.1)
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.3 * torch.randn_like(p))
    return blk.to(gpu).eval()


def _check_block_vs_float64(gpu, B, T_, D, fusable):
    import copy
    pkg, _ = _pkg()
    blk = _randomized_block(pkg, D, gpu)
    x = torch.randn(B, T_, D, device=gpu)
    assert blk._fusable(x) == fusable
    g = torch.randn(B, T_, D, device=gpu)
    xx = x.clone().requires_grad_(True)
    y = blk(xx)
    y.backward(g)
    b64 = copy.deepcopy(blk).double()
    b64.rope.rotation = blk.rope.rotation                    # the complex64 table, widened inside _rope64
    x64 = x.double().requires_grad_(True)
    y64 = _block64(b64, x64)
    y64.backward(g.double())
    c = lambda t: t.detach().cpu().numpy()
    assert rel_err(c(y), c(y64)) <= TOL
    assert rel_err(c(xx.grad), c(x64.grad)) <= TOL
    p64 = dict(b64.named_parameters())
    for name, p in blk.named_parameters():
        assert rel_err(c(p.grad), c(p64[name].grad)) <= TOL_PARAM, name


@pytest.mark.parametrize("B,T_,D", [(4, 512, 256), (8, 1024, 256), (2, 256, 1024)])
def test_fused_block_vs_float64_composition(gpu, B, T_, D):
    _check_block_vs_float64(gpu, B, T_, D, True)


def test_block_past_the_row_width_limit_vs_float64_composition(gpu):
    """D = 1026 is one pair past ENH_MAX_D: enh_supported is false, the block runs the reference's op sequence around the
    native transforms, and the numbers are still the float64 composition's.  (The other side of enh_supported, an odd
    D such as 7, has no block to check: RotaryFrequencyEmbedding pairs the channels, so the reference and this package
    both refuse an odd D before anything runs.)"""
    _, fn = _pkg()
    assert not fn.enh_supported(1026) and not fn.enh_supported(7)
    _check_block_vs_float64(gpu, 2, 64, 1026, False)


def test_misaligned_view_input(gpu):
    pkg, _ = _pkg()
    blk = _randomized_block(pkg, 64, gpu, seed=1)
    B, T_, D = 2, 256, 64
    base = torch.randn(B * T_ * D + 1, device=gpu)
    xv = base[1:].view(B, T_, D)                             # storage offset of one float: 4-byte aligned
    assert xv.data_ptr() % 16 != 0
    y_view = blk(xv)
    y_copy = blk(xv.clone())
    assert torch.equal(y_view, y_copy)
    rope = pkg.RotaryFrequencyEmbedding(D).to(gpu)
    assert torch.equal(rope(xv), rope(xv.clone()))


# ---- the three row lines through the functional API, with the library's dropout mask ---------------------------------

class _Words:
    """A DropoutState that hands out fixed (seed, counter) words."""

    def __init__(self, rng):
        self.rng, self.device = rng, rng.device

    def next(self):
        return self.rng


def _emu_masks(rng, B, n, p):
    subprocess.run(["bash", os.path.join(ROOT, "tests", "emu", "build.sh")], check=True, capture_output=True)
    emu = ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libsmx_emu.so"))
    seed, counter = (int(v) & (2**64 - 1) for v in rng.cpu().tolist())
    thr = round(p * 65536)
    out = np.zeros((B, n), np.uint8)
    for b in range(B):
        emu.emu_drop_mask(ctypes.c_ulonglong(seed), ctypes.c_ulonglong(counter), b, ctypes.c_longlong(n), thr,
                          out[b].ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))
    return torch.from_numpy(out.astype(np.float64) * (65536.0 / (65536 - thr)) if thr else np.ones((B, n)))


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _compare(got, ref):
    c = lambda t: t.detach().cpu().numpy()
    for i, (a, r) in enumerate(zip(got, ref)):
        assert rel_err(c(a), c(r)) <= (TOL if i < 4 else TOL_PARAM), i


LINE_SHAPES = [(3, 40, 6), (2, 100, 16), (4, 128, 256), (2, 64, 1024), (2, 33, 1022)]
# One width per (VEC, CH) instance of enh_dispatch that LINE_SHAPES leaves out, the power-of-two widths 128 and 512, and the widths
# one chunk past a ladder boundary, whose last chunk is nearly all padding lanes ("Which test
# reaches which row-kernel instance").  74 and 111 rows: the last block of four waves is ragged.
WIDTH_SHAPES = [(2, 37, 128),    # <4, 1>, lanes 0-31 only (the full tile of <2, 1>, which D % 4 == 0 never takes)
                (2, 37, 130),    # <2, 2>, one pair past <2, 1>
                (3, 37, 258),    # <2, 4>, one pair past <2, 2>
                (2, 37, 260),    # <4, 2>, one chunk past <4, 1>
                (2, 37, 384),    # <4, 2>
                (3, 37, 510),    # <2, 4>, one pair short of full
                (2, 37, 512),    # <4, 2> full
                (2, 37, 514),    # <2, 8>, one pair past <2, 4>
                (3, 37, 516)]    # <4, 4>, one chunk past <4, 2>
# More than LN_MAX_BLOCKS * ROW_WAVES = 8192 rows, so a wave walks several rows (accumulating the parameter gradients
# over them, with the dropout key of another batch row on a later pass), and the block counts that k_ln_colsum's three
# tiers split differently.  D = 6 is Vec<2>, D = 8 Vec<4>.
WALK_SHAPES = [(3, 2731, 8),     # 8193 rows: one wave takes a second row
               (3, 2731, 6),
               (4, 2047, 6),     # 8188 rows: 2047 blocks, just under the cap
               (4, 2047, 8),
               (2, 1200, 8),     # 2400 rows: 600 blocks = 512 + 64 + 24, the middle tier and the tail of the column sum
               (2, 1200, 6),
               (5, 4000, 6),     # 20000 rows: waves take two or three rows
               (5, 4000, 8)]


@pytest.mark.parametrize("B,T_,D", LINE_SHAPES + WIDTH_SHAPES + WALK_SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_row_lines_vs_composition_with_the_library_mask(gpu, B, T_, D, p):
    """Each line's forward and backward against autograd of the reference's op sequence in float64, with the mask
    the library documents for the same two words: the backward regenerates exactly the forward's mask."""
    pkg, fn = _pkg()
    torch.manual_seed(B + T_ + D)
    rng = fn.DropoutState(gpu).next()
    M = _emu_masks(rng, B, T_ * D, p).view(B, T_, D).to(gpu)
    ws = _Words(rng)
    n = lambda k: torch.nn.LayerNorm(k).to(gpu)
    n1, n2, n3, ng = n(D), n(D), n(D), n(2 * D)
    with torch.no_grad():
        for m in (n1, n2, n3, ng):
            m.weight.normal_(1.0, 0.3); m.bias.normal_(0.0, 0.3)
    if (B, T_, D) in WALK_SHAPES:                            # a table of exactly T rows, every row its own angles
        rot = torch.polar(torch.ones(T_, D // 2), 6.0 * torch.rand(T_, D // 2)).to(gpu)
    else:
        rot = pkg.RotaryFrequencyEmbedding(D).rotation.to(gpu)
    d = lambda t: t.detach().double().requires_grad_(True)

    # line 1: (x1, h2)
    x = torch.randn(B, T_, D, device=gpu)
    g1, gh2 = torch.randn_like(x), torch.randn_like(x)
    w = [_leaf(t) for t in (x, n1.weight, n1.bias, n2.weight, n2.bias)]
    x1, h2 = fn.rope_norm(w[0], rot, w[1], w[2], w[3], w[4], n1.eps, n2.eps, p, ws)
    ((x1 * g1).sum() + (h2 * gh2).sum()).backward()
    r = [d(t) for t in (x, n1.weight, n1.bias, n2.weight, n2.bias)]
    rx1 = r[0] + M * _rope64(rot, _ln(n1, r[0], r[1], r[2]))
    rh2 = _ln(n2, rx1, r[3], r[4])
    ((rx1 * g1.double()).sum() + (rh2 * gh2.double()).sum()).backward()
    _compare([x1, h2, w[0].grad, w[0].grad] + [t.grad for t in w[1:]],
             [rx1, rh2, r[0].grad, r[0].grad] + [t.grad for t in r[1:]])

    # line 2's residual and norm3: (x2, h3)
    pin = torch.randn_like(x)
    w = [_leaf(t) for t in (x, pin, n3.weight, n3.bias)]
    x2, h3 = fn.residual_norm(w[0], w[1], w[2], w[3], n3.eps, p, ws)
    ((x2 * g1).sum() + (h3 * gh2).sum()).backward()
    r = [d(t) for t in (x, pin, n3.weight, n3.bias)]
    rx2 = r[0] + M * r[1]
    rh3 = _ln(n3, rx2, r[2], r[3])
    ((rx2 * g1.double()).sum() + (rh3 * gh2.double()).sum()).backward()
    _compare([x2, h3, w[0].grad, w[1].grad, w[2].grad, w[3].grad],
             [rx2, rh3, r[0].grad, r[1].grad, r[2].grad, r[3].grad])

    # line 3 after the Linears: x3
    a, v = torch.randn(B, T_, 2 * D, device=gpu), torch.randn_like(x)
    w = [_leaf(t) for t in (a, v, x, ng.weight, ng.bias)]
    x3 = fn.gate_blend(w[0], w[1], w[2], w[3], w[4], ng.eps, p, ws)
    x3.backward(g1)
    r = [d(t) for t in (a, v, x, ng.weight, ng.bias)]
    gate, vt = F.layer_norm(r[0], (2 * D,), r[3], r[4], ng.eps).chunk(2, dim=-1)
    gate = torch.sigmoid(gate)
    rx3 = r[2] + M * (gate * r[1] + (1 - gate) * vt)
    rx3.backward(g1.double())
    _compare([x3, w[0].grad, w[1].grad, w[2].grad, w[3].grad, w[4].grad],
             [rx3, r[0].grad, r[1].grad, r[2].grad, r[3].grad, r[4].grad])


def test_drop_fraction_of_each_line(gpu):
    _, fn = _pkg()
    p, B, T_, D = 0.3, 8, 1024, 256
    ds = fn.DropoutState(gpu)
    x = torch.randn(B, T_, D, device=gpu)
    rot = torch.polar(torch.ones(4096, D // 2), torch.randn(4096, D // 2)).to(gpu)
    ones = torch.ones(D, device=gpu)
    zeros = torch.zeros(D, device=gpu)
    x1, _ = fn.rope_norm(x, rot, ones, zeros, ones, zeros, 1e-5, 1e-5, p, ds)
    x2, _ = fn.residual_norm(x, torch.ones_like(x), ones, zeros, 1e-5, p, ds)
    a = torch.randn(B, T_, 2 * D, device=gpu)
    x3 = fn.gate_blend(a, torch.full_like(x, 5.0), x, None, None, 1e-5, p, ds)
    for y in (x1, x2, x3):
        frac = ((y - x) == 0).float().mean().item()
        assert abs(frac - p) < 0.01, frac
    assert not torch.equal(x2 == x, x3 == x)                 # every line draws its own words


def _check_row_backward_reproducible(gpu, B, T_, D):
    _, fn = _pkg()
    torch.manual_seed(5)
    x, pin = torch.randn(B, T_, D, device=gpu), torch.randn(B, T_, D, device=gpu)
    a = torch.randn(B, T_, 2 * D, device=gpu)
    rot = torch.polar(torch.ones(T_, D // 2), torch.randn(T_, D // 2)).to(gpu)
    prm = [torch.randn(k, device=gpu) for k in (D, D, D, D, D, D, 2 * D, 2 * D)]
    g = torch.randn(B, T_, D, device=gpu)

    def run():
        w = [_leaf(t) for t in [x, pin, a] + prm]
        x1, h2 = fn.rope_norm(w[0], rot, w[3], w[4], w[5], w[6], 1e-5, 1e-5)
        x2, h3 = fn.residual_norm(x1, w[1] * h2, w[7], w[8], 1e-5)
        x3 = fn.gate_blend(w[2], h3, x2, w[9], w[10], 1e-5)
        x3.backward(g)
        torch.cuda.synchronize()
        return [t.grad.clone() for t in w]

    first, second = run(), run()
    for i, (u, v) in enumerate(zip(first, second)):
        assert torch.equal(u, v), i


def test_row_backward_is_bitwise_reproducible(gpu):
    _check_row_backward_reproducible(gpu, 16, 512, 256)


def test_row_backward_is_bitwise_reproducible_on_the_row_walk(gpu):
    """20000 rows: every wave adds two or three rows into its partial sums before the block reduction"""
    _check_row_backward_reproducible(gpu, 5, 4000, 8)


def test_fuse_dropout_off_matches_the_composition_with_torch_masks(gpu):
    pkg, _ = _pkg()
    blk = _randomized_block(pkg, 64, gpu, seed=2).train()
    blk.dropout.p = 0.25
    x = torch.randn(2, 256, 64, device=gpu)
    blk.fuse_dropout = False
    assert not blk._fusable(x)
    torch.manual_seed(11)
    y = blk(x)
    torch.manual_seed(11)
    dr = blk.dropout
    h = x + dr(blk.rope(blk.norm1(x)))
    h = h + dr(blk.phase_mixing(blk.norm2(h)))
    h = h + dr(blk.gated(blk.norm3(h)))
    ref = h + dr(blk.multi_scale(h))
    assert torch.equal(y, ref)
    blk.fuse_dropout = True
    assert blk._fusable(x)
    yf = blk(x)
    blk.eval()
    assert not torch.equal(yf, blk(x))                        # training mode does drop on the fused path


def test_graph_replay_equals_eager(gpu):
    pkg, _ = _pkg()
    blk = _randomized_block(pkg, 256, gpu, seed=3)
    x = torch.randn(4, 512, 256, device=gpu, requires_grad=True)
    g = torch.randn(4, 512, 256, device=gpu)

    def step():
        for p in blk.parameters():
            p.grad = None
        x.grad = None
        y = blk(x)
        y.backward(g)
        return y

    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        for _ in range(2):
            step()                                           # tables, workspaces, autotuned GEMMs
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize()
    ye = step().detach().clone()
    ge = [x.grad.clone()] + [p.grad.clone() for p in blk.parameters()]
    for p in blk.parameters():
        p.grad = None
    x.grad = None
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        yg = blk(x)
        yg.backward(g)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.allclose(yg, ye, rtol=0, atol=1e-6 * float(ye.abs().max()))
    for a, b in zip([x.grad] + [p.grad for p in blk.parameters()], ge):
        assert torch.allclose(a, b, rtol=0, atol=1e-5 * float(b.abs().max()) + 1e-30)


def test_drop_in_model_trains_a_step(gpu):
    """benchmark_enhanced.py's EnhancedSpectralLanguageModel, built on this package's block."""
    pkg, _ = _pkg()

    class Model(torch.nn.Module):
        def __init__(self, embed_dim=256, num_layers=4):
            super().__init__()
            self.byte_proj = torch.nn.Linear(256, embed_dim)
            self.layers = torch.nn.ModuleList([pkg.EnhancedSpectralBlock(embed_dim) for _ in range(num_layers)])
            self.norm = torch.nn.LayerNorm(embed_dim)
            self.output = torch.nn.Linear(embed_dim, 256)

        def forward(self, byte_ids):
            x = self.byte_proj(F.one_hot(byte_ids, num_classes=256).float())
            for layer in self.layers:
                x = layer(x)
            return self.output(self.norm(x))

    torch.manual_seed(0)
    model = Model().to(gpu).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    ids = torch.randint(0, 256, (4, 513), device=gpu)
    losses = []
    for _ in range(3):
        logits = model(ids[:, :-1])
        loss = F.cross_entropy(logits.reshape(-1, 256), ids[:, 1:].reshape(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
