#!/usr/bin/env python3
"""Golden vectors of fft_tensor/optimized_ops.py and fft_tensor/production_ready.py, produced by the REFERENCE modules on
the CPU.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_optops.py

One file per convolution case of optops_common.CONV1D / CONV2D (optops_common.conv1d_name / conv2d_name) holding
  out               the reference's fp32 result of fast_frequency_conv1d / fast_frequency_conv2d
  ref_err           its max-normalised error against optops_common.conv1d_def / conv2d_def (float64)
  x_sum, w_sum      float64 sums of the inputs, which the tests draw again from optops_common.conv*_inputs (the weights of
                    the larger cases alone would be hundreds of KiB)
and O20_optops_members.npz with the other members: topk.*, sfft.*, sifft.*, matmul.*, linear.* (a state_dict, an input,
the forward result and the gradients of weight_freq and bias under the recorded upstream gradient), compress.*, bsm.*,
smart.*, osst.* and `signatures`, the inspect.signature string of every public member (optops_common.MEMBERS).
The generator FAILS if a convolution's own error exceeds half of TOL_ACT (the single-sample case O04 is one product x[0] w[0]
held against the rounding of a whole 256-point circular product, so its max-normalised error is the largest)."""
import contextlib
import inspect
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                     # noqa: E402  (puts the reference on sys.path)
import optops_common as oc                                   # noqa: E402
from conftest import TOL_ACT, rel_err                        # noqa: E402

warnings.filterwarnings("ignore")
with contextlib.redirect_stdout(io.StringIO()):
    from fft_tensor import optimized_ops as ref_opt          # noqa: E402
    from fft_tensor import production_ready as ref_prod      # noqa: E402

O = ref_opt.OptimizedFrequencyOps


def conv_record(out, out64, x, w):
    e = rel_err(out.numpy(), out64.numpy())
    assert e <= TOL_ACT / 2, e
    return {"out": out, "ref_err": np.float64(e), "x_sum": np.float64(x.double().sum()), "w_sum": np.float64(w.double().sum())}


def signature_of(cls, name):
    fn = inspect.getattr_static(cls, name)
    fn = getattr(fn, "__func__", fn)
    fn = getattr(fn, "__wrapped__", fn)
    try:
        return str(inspect.signature(fn))
    except (TypeError, ValueError):                           # a torch.jit.script function: its schema names the arguments
        args = fn.schema.arguments
        return "(" + ", ".join(f"{a.name}: {'torch.Tensor' if str(a.type) == 'Tensor' else str(a.type)}" for a in args) + ")"


def members():
    gen = torch.Generator().manual_seed(oc.SEED)
    rec = {}
    # top-k on a complex tensor with separated magnitudes
    data = oc.separated_spectrum((6, 50), 40)
    v, i = O.fast_topk_sparse(data, 40)
    rec.update({"topk.data": data, "topk.k": np.int64(40), "topk.values": v, "topk.indices": i})
    # sparse fft / ifft of a complex input whose spectrum is separated
    sp = oc.spatial_with_separated_spectrum((8, 12))
    c, idx = O.optimized_sparse_fft(sp, 0.25)
    oc.assert_separated(torch.fft.fftn(sp), c.numel())
    rec.update({"sfft.x": sp, "sfft.sparsity": np.float64(0.25), "sfft.coeffs": c, "sfft.indices": idx,
                "sifft.out": O.optimized_sparse_ifft(c, idx, (8, 12), device="cpu")})
    xr = torch.randn(5, 9, generator=gen)                     # and of a real one (Hermitian pairs: the set is what counts)
    cr, ir = O.optimized_sparse_fft(xr, 0.2)
    rec.update({"sfft.real.x": xr, "sfft.real.coeffs": cr, "sfft.real.indices": ir,
                "sifft.real.out": O.optimized_sparse_ifft(cr, ir, (5, 9), device="cpu")})
    # matmul (the whole-weight branch; the block branch needs a 100 MB weight: GPU test)
    x = torch.randn(2, 5, 12, generator=gen)
    wf = oc.crandn(gen, 12, 20)
    out = O.fast_frequency_matmul(x, wf)
    rec.update({"matmul.x": x, "matmul.w_freq": wf, "matmul.out": out,
                "matmul.ref_err": np.float64(rel_err(out.numpy(), oc.matmul_def(x, wf).numpy()))})
    # the linear layer
    torch.manual_seed(oc.SEED)
    lin = ref_opt.ProductionFrequencyLinear(48, 10, sparsity=0.25)
    with torch.no_grad():
        lin.bias.copy_(0.1 * torch.randn(10, generator=gen))
    lx = torch.randn(3, 7, 48, generator=gen)
    lg = torch.randn(3, 7, 10, generator=gen)
    ly = lin(lx)
    ly.backward(lg)
    rec.update({"linear.seed": np.int64(oc.SEED), "linear.x": lx, "linear.g": lg, "linear.out": ly,
                "linear.grad_weight_freq": lin.weight_freq.grad, "linear.grad_bias": lin.bias.grad})
    rec.update({"linear.state." + k: t for k, t in lin.state_dict().items()})
    # production_ready
    t = torch.randn(16, 24, generator=gen)
    comp = ref_prod.ProductionFrequencyOps.compress_tensor(t, sparsity=0.2)
    bx = torch.randn(2, 3, 16, generator=gen)
    rec.update({"compress.x": t, "compress.sparsity": np.float64(0.2), "compress.indices": comp.indices.numpy().astype(np.int16),
                "compress.freq_coeffs": comp.freq_coeffs, "compress.to_spatial": comp.to_spatial(),
                "bsm.x": bx, "bsm.block_size": np.int64(10),
                "bsm.out": ref_prod.ProductionFrequencyOps.block_streaming_matmul(bx, comp, block_size=10)})
    cx, cw = torch.randn(1, 2, 14, 15, generator=gen), torch.randn(3, 2, 12, 12, generator=gen)
    rec.update({"smart.x": cx, "smart.w": cw, "smart.out": ref_prod.ProductionFrequencyOps.smart_conv2d(cx, cw, padding=1)})
    o = ref_prod.OptimizedSparseSpectralTensor(data=t, sparsity=0.2, device="cpu")
    first = o.to_spatial()
    assert o.to_spatial() is first
    rec["osst.to_spatial"] = first
    sigs = []
    for cls, names in oc.MEMBERS.items():
        owner = getattr(ref_opt, cls, None) or getattr(ref_prod, cls)
        sigs += [f"{cls}.{n}{signature_of(owner, n)}" for n in names]
    rec["signatures"] = np.array(sigs)
    mg.save("O20_optops_members", rec)
    print("\n".join(sigs))


if __name__ == "__main__":
    for i, case in enumerate(oc.CONV1D):
        x, w = oc.conv1d_inputs(case)
        out = O.fast_frequency_conv1d(x, w, stride=case[6], padding=case[5])
        r = conv_record(out, oc.conv1d_def(x, w, case[6], case[5]), x, w)
        print(oc.conv1d_name(i), "reference error %.2e" % r["ref_err"])
        mg.save(oc.conv1d_name(i), r)
    for i, case in enumerate(oc.CONV2D):
        x, w = oc.conv2d_inputs(case)
        out = O.fast_frequency_conv2d(x, w, stride=case[8], padding=case[7])
        r = conv_record(out, oc.conv2d_def(x, w, case[8], case[7]), x, w)
        print(oc.conv2d_name(i), "reference error %.2e" % r["ref_err"])
        mg.save(oc.conv2d_name(i), r)
    members()
