"""The store layout (option "st_layout": WHICH of a thread's 16 rows per tile go out with the write-back policy) and the
count (option "st_plain": how many) are cache policy only: for every layout x count the forward y and the backward
grad_x, grad_w_real, grad_w_imag, grad_bias must be bitwise what (layout -1, same count) gives, on every kernel that
stores through store_rows (csrc/smx_launch.h) and with every source of the rotation s (tile residue r, r >> 2, wave).
Each case asserts the plan it means to reach and checks the (-1, automatic count) result once against the oracle at
the suite's stated tolerance.  The pure-Python model of the masks is tests/test_store_layout_cpu.py.
"""

import numpy as np
import pytest
import torch

from conftest import TOL_ACT, TOL_PARAM, rel_err
from oracle import spectral_oracle as so

pytestmark = pytest.mark.gpu

LAYOUTS = (-1, 0, 1, 2, 3, 4)
COUNTS = (0, 1, 2, 4)


def _mods():
    import tensor_cuda_fft_amd as pkg
    from tensor_cuda_fft_amd import _lib, functional
    return pkg, _lib, functional


def _restore(_lib):
    _lib.set_option("st_layout", -2)
    _lib.set_option("st_plain", -1)
    _lib.set_option("nsplit", 0)


def _layer(pkg, D, F, dev, p=0.0):
    torch.manual_seed(5)
    layer = pkg.SpectralMixingLayer(D, num_filters=F, dropout=p).to(dev)
    with torch.no_grad():
        layer.weight_real.normal_(1.0, 0.5)
        layer.weight_imag.normal_(0.0, 0.5)
        layer.bias.normal_(0.5, 0.1)
    return layer


def _run_layer(layer, x, g):
    """fwd + bwd; seeded before the forward so that a training-mode call draws the same dropout mask every time"""
    x = x.detach().clone().requires_grad_(True)
    for q in layer.parameters():
        q.grad = None
    torch.manual_seed(11)
    y = layer(x)
    y.backward(g)
    torch.cuda.synchronize()
    return (y.detach(), x.grad.detach(), layer.weight_real.grad.clone(), layer.weight_imag.grad.clone(),
            layer.bias.grad.clone())


def _sweep(_lib, run):
    """run() under every layout x count; every result bitwise equal to the one under (-1, same count).  Returns the
    result under (-1, automatic count).  The caller restores the options."""
    _lib.set_option("st_layout", -1)
    _lib.set_option("st_plain", -1)
    auto = run()
    for count in COUNTS:
        _lib.set_option("st_plain", count)
        _lib.set_option("st_layout", -1)
        base = run()
        for a, b in zip(base, auto):           # nor does the count change a bit
            assert torch.equal(a, b), f"count {count} against the automatic count"
        for layout in LAYOUTS[1:]:
            _lib.set_option("st_layout", layout)
            got = run()
            for name, a, b in zip(("y", "grad_x", "grad_w_real", "grad_w_imag", "grad_bias"), got, base):
                assert a.dtype == b.dtype and torch.equal(a, b), f"{name}: layout {layout}, count {count}"
        # the two directions take the operand separately
        _lib.set_option("st_layout_fwd", 1)
        _lib.set_option("st_layout_bwd", 3)
        got = run()
        for a, b in zip(got, base):
            assert torch.equal(a, b), f"fwd 1 / bwd 3, count {count}"
    return auto


def _check_oracle(got, x, g, layer, tol_act=TOL_ACT):
    c = lambda t: t.detach().float().cpu().numpy()
    wr, wi, b = c(layer.weight_real), c(layer.weight_imag), c(layer.bias)
    y_ref, _ = so.forward_closed(c(x), wr, wi, b)
    gx_ref, gwr_ref, gwi_ref, gb_ref = so.backward_closed(c(x), wr, wi, c(g))
    y, gx, gwr, gwi, gb = got
    assert rel_err(c(y), y_ref) <= tol_act and rel_err(c(gx), gx_ref) <= tol_act
    assert rel_err(c(gwr), gwr_ref) <= TOL_PARAM and rel_err(c(gwi), gwi_ref) <= TOL_PARAM
    assert rel_err(c(gb), gb_ref) <= TOL_PARAM


LAYER_CASES = [  # (B, N, D, F), nsplit option, (bands, L), split plan?
    ((2, 2048, 64, 16), 1, (1, 8), False),     # fused plan, L = 8: r >> 2 takes two values, r eight; two d-tiles
    ((2, 4096, 48, 128), 1, (1, 16), False),   # L = 16; ragged D: lanes past D dropped by the buffer range
    ((2, 4096, 64, 128), 0, (1, 16), True),    # the plan rule picks the residue-split plan (k_split_b) on its own
    ((2, 1024, 64, 256), 1, (2, 4), False),    # two bands (k_fused<2, .>)
]


@pytest.mark.parametrize("shape,nsplit,bl,split", LAYER_CASES, ids=["x".join(map(str, c[0])) for c in LAYER_CASES])
def test_layer_bitwise_under_every_layout(gpu, shape, nsplit, bl, split):
    pkg, _lib, _ = _mods()
    B, N, D, F = shape
    try:
        _lib.set_option("nsplit", nsplit)
        p = _lib.plan(B, N, D, F)
        assert (p.path, p.bands, p.L, p.groups) == (_lib.SMX_PATH_DECIMATED, bl[0], bl[1], 1)
        assert (p.nsplit > 1) if split else (p.nsplit == 1)
        layer = _layer(pkg, D, F, gpu)
        torch.manual_seed(1)
        x = torch.randn(B, N, D, device=gpu)
        g = torch.randn(B, N, D, device=gpu)
        auto = _sweep(_lib, lambda: _run_layer(layer, x, g))
        _check_oracle(auto, x, g, layer)
    finally:
        _restore(_lib)


def test_zero_padded_rows_bitwise_under_every_layout(gpu):
    """spectral_filter with n_fft above the row count: the PAD instantiation (the row pitch in the per-lane offset)"""
    _, _lib, fn = _mods()
    B, R, D, F, n_fft, k = 4, 600, 64, 60, 1024, 60
    try:
        _lib.set_option("nsplit", 1)
        p = _lib.plan_ex(_lib.smx_shape(B, R, D, F, n_fft, k))
        assert (p.path, p.bands, p.L, p.nsplit, p.groups) == (_lib.SMX_PATH_DECIMATED, 1, 4, 1, 1)
        rng = np.random.default_rng(3)
        x, g = (rng.standard_normal((B, R, D)).astype(np.float32) for _ in range(2))
        wr = (1 + 0.5 * rng.standard_normal((D, F))).astype(np.float32)
        wi = (0.5 * rng.standard_normal((D, F))).astype(np.float32)
        b = (0.1 * rng.standard_normal(D)).astype(np.float32)
        T = torch.from_numpy

        def run():
            xd, wrd, wid, bd = (T(a).to(gpu).requires_grad_(True) for a in (x, wr, wi, b))
            y = fn.spectral_filter(xd, wrd, wid, bd, n_fft=n_fft, k=k)
            y.backward(T(g).to(gpu))
            torch.cuda.synchronize()
            return y.detach(), xd.grad, wrd.grad, wid.grad, bd.grad

        y, gx, gwr, gwi, gb = (t.cpu().numpy() for t in _sweep(_lib, run))
        y_ref, _ = so.forward_closed_ex(x, wr, wi, b, n_fft, k)
        gx_ref, gwr_ref, gwi_ref, gb_ref = so.backward_closed_ex(x, wr, wi, g, n_fft, k)
        assert rel_err(y, y_ref) <= TOL_ACT and rel_err(gx, gx_ref) <= TOL_ACT
        assert rel_err(gwr, gwr_ref) <= TOL_PARAM and rel_err(gwi, gwi_ref) <= TOL_PARAM
        assert rel_err(gb, gb_ref) <= TOL_PARAM
    finally:
        _restore(_lib)


def test_bf16_rows_bitwise_under_every_layout(gpu):
    """2-byte rows: buffer_store_dword instead of dwordx2 carries the same mask.  Oracle bound: y and grad_x are the
    f32 results rounded once to bf16 (8 significant bits: half an ulp is 2^-9 of the element, so at most 2^-9 of the
    largest one) on top of the f32 path's 1e-5, under 2^-8 as in test_half_io_gpu; the parameter gradients stay f32."""
    pkg, _lib, _ = _mods()
    B, N, D, F = 8, 1024, 64, 32
    try:
        _lib.set_option("nsplit", 1)
        p = _lib.plan(B, N, D, F)
        assert (p.path, p.bands, p.L, p.nsplit, p.groups) == (_lib.SMX_PATH_DECIMATED, 1, 4, 1, 1)
        assert _lib.io_supported(B, N, D, F, _lib.SMX_IO_BF16)
        layer = _layer(pkg, D, F, gpu)
        torch.manual_seed(1)
        x = torch.randn(B, N, D, device=gpu).to(torch.bfloat16)
        g = torch.randn(B, N, D, device=gpu).to(torch.bfloat16)
        auto = _sweep(_lib, lambda: _run_layer(layer, x, g))
        assert auto[0].dtype == torch.bfloat16 and auto[1].dtype == torch.bfloat16
        _check_oracle(auto, x, g, layer, tol_act=2.0 ** -8)
    finally:
        _restore(_lib)


def test_dropout_bitwise_under_every_layout(gpu):
    """p = 0.25, seeded: the DROP instantiations (mask on the stored tile forward, on the loaded g backward).  Against
    the oracle: the training-mode result is the oracle's y under the mask the launch drew, and its gradients are the
    oracle's for g * mask * scale."""
    pkg, _lib, _ = _mods()
    B, N, D, F, pdrop = 4, 2048, 64, 32, 0.25
    try:
        _lib.set_option("nsplit", 1)
        p = _lib.plan(B, N, D, F)
        assert (p.path, p.bands, p.L, p.nsplit, p.groups) == (_lib.SMX_PATH_DECIMATED, 1, 8, 1, 1)
        layer = _layer(pkg, D, F, gpu, p=pdrop)
        layer.train()
        torch.manual_seed(1)
        x = torch.randn(B, N, D, device=gpu)
        g = torch.randn(B, N, D, device=gpu)
        y, gx, gwr, gwi, gb = _sweep(_lib, lambda: _run_layer(layer, x, g))
        c = lambda t: t.detach().cpu().numpy()
        mask = c(y) != 0                       # (the bias keeps y away from an exact zero)
        thr = round(pdrop * 65536)
        keep = 1.0 - thr / 65536.0
        assert abs(mask.mean() - keep) <= 5.0 * (keep * (1 - keep) / mask.size) ** 0.5 + 1e-3
        wr, wi, b = c(layer.weight_real), c(layer.weight_imag), c(layer.bias)
        y_ref, _ = so.forward_closed(c(x), wr, wi, b)
        assert rel_err(c(y), np.where(mask, y_ref / keep, 0.0)) <= TOL_ACT
        gx_ref, gwr_ref, gwi_ref, gb_ref = so.backward_closed(c(x), wr, wi, c(g) * mask / keep)
        assert rel_err(c(gx), gx_ref) <= TOL_ACT
        assert rel_err(c(gwr), gwr_ref) <= TOL_PARAM and rel_err(c(gwi), gwi_ref) <= TOL_PARAM
        assert rel_err(c(gb), gb_ref) <= TOL_PARAM
    finally:
        _restore(_lib)
