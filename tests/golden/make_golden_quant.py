#!/usr/bin/env python3
"""Golden vectors of fft_tensor/polar_quantization.py, fft_tensor/zero_materialize.py and the offline half of
fft_tensor/llamaizer.py, produced by the REFERENCE modules on the CPU.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_quant.py

R11..R13_polar_<shape>.npz, one per quant_common.POLAR_SHAPES (the input is drawn again by quant_common.polar_input; z_sum
checks it), with, per config "<mag_bits>_<phase_bits>" of POLAR_CONFIGS:
  range.<c>                     the reference's mag_range (two floats)
  mag_q.<c>, phase_q.<c>        its codes
  deq.<c>                       its dequantize of them (the two smaller shapes only: a function of the codes)
  rt_err.<c>                    ||dequantize(quantize(z)) - z|| / ||z||, the error of the FORMAT
  deq_err.<c>                   max-normalised error of its dequantize against quant_common.polar_dequantize_def
  ref_flips.<c>, ref_worst.<c>  how many of its (mag, phase) codes differ from the float64 codes and the largest distance
                                from a rounding boundary at which one does (quant_common.check_codes; the generator FAILS
                                beyond BAND / 10)
R21_log8.npz: x / enc / ref_flips / ref_worst for quant_common.log8_input((3, 1000)), dec of all 256 codes with dec_err (the
largest relative error against float64), and the complex pair c.z, c.re_q, c.im_q, c.indices, c.out (decompress into (64,)).
R31_zero_materialize.npz: signatures; layer.<seed>.<learn_phase>.state.*, .x, .out, .ratio; linear.*, conv1d.<i>.*, conv2d.*,
conv3d.* (out and ref_err against quant_common's complex128 definitions); wirtinger.*; convert.* (an nn.Linear's weight and
bias and the converted state for both learn_phase values)."""
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
import quant_common as qc                                    # noqa: E402
from conftest import TOL_ACT, rel_err                        # noqa: E402

warnings.filterwarnings("ignore")
with contextlib.redirect_stdout(io.StringIO()):
    from fft_tensor import llamaizer as ref_ll               # noqa: E402
    from fft_tensor import polar_quantization as ref_pq      # noqa: E402
    from fft_tensor import zero_materialize as ref_zm        # noqa: E402

C = ref_zm.ConvolutionTheoremMatMul


def polar():
    for shape in qc.POLAR_SHAPES:
        z = qc.polar_input(shape)
        rec = {"z_sum": np.complex128(z.to(torch.complex128).sum())}
        for mb, pb in qc.POLAR_CONFIGS:
            c = f"{mb}_{pb}"
            q = ref_pq.PolarQuantizer(mb, pb)
            mag_q, phase_q = q.quantize(z)
            deq = q.dequantize(mag_q, phase_q)
            u, v = qc.polar_uv_def(z, mb, pb, q.mag_range)
            assert max(qc.band_share(u, "round"), qc.band_share(v, "round")) <= qc.BAND_SHARE
            flips, worst = 0, 0.0
            if pb <= 8:                                       # above 8 bits the uint8 cast wraps: no code to compare
                fm, wm = qc.check_codes(mag_q, u, 2 ** mb - 1, "round", qc.BAND / 10)
                fp, wp = qc.check_codes(phase_q, v, 2 ** pb - 1, "round", qc.BAND / 10)
                flips, worst = (fm, fp), max(wm, wp)
            rec.update({f"range.{c}": np.float64(q.mag_range), f"mag_q.{c}": mag_q, f"phase_q.{c}": phase_q,
                        f"rt_err.{c}": np.float64((torch.norm(deq - z) / torch.norm(z)).item()),
                        f"deq_err.{c}": np.float64(rel_err(deq.numpy(), qc.polar_dequantize_def(mag_q, phase_q, mb, pb,
                                                                                                q.mag_range))),
                        f"ref_flips.{c}": np.int64(flips), f"ref_worst.{c}": np.float64(worst)})
            if z.numel() <= 5000:
                rec[f"deq.{c}"] = deq
            print(qc.polar_name(shape), c, "rt %.4f deq_err %.2e flips %s worst %.2e"
                  % (rec[f"rt_err.{c}"], rec[f"deq_err.{c}"], flips, worst))
        mg.save(qc.polar_name(shape), rec)


def log8():
    Q = ref_zm.LogarithmicQuantizer
    x = qc.log8_input((3, 1000))
    enc = Q.log8_encode(x)
    sign, t = qc.log8_t_def(x)
    assert qc.band_share(t, "trunc") <= qc.BAND_SHARE
    assert np.array_equal((enc.numpy() >> 7).astype(np.int64), sign)
    flips, worst = qc.check_codes(enc & 127, t, 127, "trunc", qc.BAND / 10)
    codes = torch.arange(256, dtype=torch.uint8)
    dec = Q.log8_decode(codes)
    dec_err = float(np.max(np.abs(dec.numpy().astype(np.float64) / qc.log8_decode_def(codes) - 1)))
    g = torch.Generator().manual_seed(qc.SEED)
    z = qc.crandn(g, 20) * 10.0 ** (torch.rand(20, generator=g) * 4 - 2)
    idx = torch.randperm(64, generator=g)[:20]
    re_q, im_q = Q.compress_sparse_freq(z, idx)
    out = Q.decompress_sparse_freq(re_q, im_q, idx, (64,))
    print("log8 flips %d worst %.2e dec_err %.2e" % (flips, worst, dec_err))
    mg.save("R21_log8", {"x": x, "enc": enc, "ref_flips": np.int64(flips), "ref_worst": np.float64(worst), "dec": dec,
                         "dec_err": np.float64(dec_err), "c.z": z, "c.re_q": re_q, "c.im_q": im_q, "c.indices": idx,
                         "c.out": out})


def signature_of(owner, name):
    fn = inspect.getattr_static(owner, name) if isinstance(owner, type) else getattr(owner, name)
    fn = getattr(fn, "__func__", fn)
    return str(inspect.signature(fn))


def conv_rec(prefix, out, x, w, stride, padding):
    e = rel_err(out.numpy(), qc.conv_def(x, w, stride, padding).numpy()) if out.numel() else 0.0
    assert e <= TOL_ACT / 2, e
    print(prefix, tuple(out.shape), "reference error %.2e" % e)
    return {prefix + ".x": x, prefix + ".w": w, prefix + ".out": out, prefix + ".ref_err": np.float64(e)}


def zero_materialize():
    rec = {}
    for seed in qc.LAYER_SEEDS:
        for lp in (True, False):
            torch.manual_seed(seed)
            layer = ref_zm.FrequencyLinearLayer(qc.LAYER_ARGS[0], qc.LAYER_ARGS[1], sparsity=qc.LAYER_ARGS[2], learn_phase=lp)
            p = f"layer.{seed}.{int(lp)}"
            rec.update({f"{p}.state.{k}": v for k, v in layer.state_dict().items()})
            x = torch.randn(2, 3, qc.LAYER_ARGS[0], generator=torch.Generator().manual_seed(qc.SEED + seed))
            rec.update({p + ".x": x, p + ".out": layer(x)})
            if lp:
                rec[p + ".ratio"] = np.float64(layer.compress_ratio())
    x, w, b = qc.linear_inputs(*qc.LINEAR)
    out = C.frequency_linear(x, w, b)
    rec.update({"linear.x": x, "linear.w": w, "linear.bias": b, "linear.out": out,
                "linear.batched": C.frequency_linear_batched(x, w, b, chunk_size=1),
                "linear.ref_err": np.float64(rel_err(out.numpy(), qc.linear_def(x, w, b).numpy()))})
    print("linear reference error %.2e" % rec["linear.ref_err"])
    for i, case in enumerate(qc.CONV1D):
        x, w = qc.conv1d_inputs(case)
        rec.update(conv_rec(f"conv1d.{i}", C.frequency_conv1d(x, w, stride=case[6], padding=case[5]), x, w, case[6], case[5]))
    x, w = qc.conv2d_inputs()
    rec.update(conv_rec("conv2d", C.frequency_conv2d(x, w, stride=qc.CONV2D[8], padding=qc.CONV2D[7]), x, w, qc.CONV2D[8],
                        qc.CONV2D[7]))
    x, w = qc.conv3d_inputs()
    rec.update(conv_rec("conv3d", C.frequency_conv3d(x, w), x, w, (1, 1, 1), (0, 0, 0)))
    g = torch.Generator().manual_seed(qc.SEED + 11)
    a, bb, go = (qc.crandn(g, 4, 6) for _ in range(3))
    a.requires_grad_(True)
    bb.requires_grad_(True)
    y = ref_zm.WirtingerAutograd.apply(a, bb)
    y.backward(go)
    rec.update({"wirtinger.x": a.detach(), "wirtinger.w": bb.detach(), "wirtinger.g": go, "wirtinger.out": y.detach(),
                "wirtinger.grad_x": a.grad, "wirtinger.grad_w": bb.grad})
    torch.manual_seed(qc.SEED)
    lin = torch.nn.Linear(128, 128)
    rec.update({"convert.weight": lin.weight.detach(), "convert.bias": lin.bias.detach()})
    for lp in (True, False):
        conv = ref_ll.FFTConverter.convert_linear_to_frequency(lin, sparsity=0.1, learn_phase=lp)
        rec.update({f"convert.{int(lp)}.{k}": v for k, v in conv.state_dict().items()})
    sigs = []
    for cls, names in qc.MEMBERS.items():
        owner = next((getattr(m, cls) for m in (ref_pq, ref_zm, ref_ll) if hasattr(m, cls)), ref_zm) if cls else ref_zm
        sigs += [f"{cls}.{n}{signature_of(owner, n)}" for n in names]
    rec["signatures"] = np.array(sigs)
    mg.save("R31_zero_materialize", rec)
    print("\n".join(sigs))


if __name__ == "__main__":
    polar()
    log8()
    zero_materialize()
