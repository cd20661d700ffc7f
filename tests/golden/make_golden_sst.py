#!/usr/bin/env python3
"""Golden vectors of the sparse spectral tensor, produced by the REFERENCE on CPU (fft_tensor.tensor, fft_tensor.ops,
fft_tensor.frequency_ops).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sst.py

One file per shape of sst_common.SHAPES and seed of sst_common.SEEDS (sst_common.golden_name), holding
  x                 torch.randn(shape, generator=torch.Generator().manual_seed(seed))
  spectrum          the complex64 spectrum the reference sparsifies (the result of its own fft.fftn call, recorded)
and per sparsity of sst_common.SPARSITIES, under the prefix sst_common.sp_tag(sparsity) + ".":
  indices (int16), freq_coeffs, to_spatial           of sst(x, sparsity, device='cpu')
  normalize                                          freq_coeffs of spectral_normalize of it
  act.indices, act.freq_coeffs                       of spectral_activation of it (`act_name`: relu at seed 1, tanh at 2)
  pool.indices, pool.freq_coeffs, pool.sparsity      of spectral_pool of it (2-D shapes; `pool_mode`: max at seed 1, avg at 2)
The (32, 32) seed-1 file also holds one FrequencyMatMul.block_streaming_matmul case: bsm.x (2, 3, 32), bsm.block_size,
bsm.sparsity, bsm.out.

While recording, every kept set is held against sst_common's numpy definition (the squared key) under
sst_common.check_membership: membership may differ only within BAND of the reference threshold, and at most BAND_CAP
entries of the spectrum lie in that band."""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                     # noqa: E402,F401  (puts the reference on sys.path)
import sst_common as sc                                      # noqa: E402

warnings.filterwarnings("ignore")
with contextlib.redirect_stdout(io.StringIO()):
    from fft_tensor import tensor as ref_tensor              # noqa: E402
    from fft_tensor import ops as ref_ops                    # noqa: E402
    from fft_tensor.frequency_ops import FrequencyMatMul     # noqa: E402


@contextlib.contextmanager
def recorded_spectra(into: list):
    """every result of the reference's fft.fftn call inside the block, in call order"""
    real = ref_tensor.fft.fftn

    def fftn(*a, **k):
        out = real(*a, **k)
        into.append(out.clone())
        return out
    ref_tensor.fft.fftn = fftn
    try:
        yield
    finally:
        ref_tensor.fft.fftn = real


def reference_sst(make):
    """(the tensor `make()` returns, the spectrum it sparsified)"""
    spectra = []
    with recorded_spectra(spectra):
        t = make()
    return t, spectra[-1]


def check_against_definition(t, spectrum, what):
    """the band rule, asserted when recording"""
    spec = spectrum.numpy().reshape(-1)
    flat = np.ravel_multi_index(tuple(t.indices.numpy().T), t.shape)
    k = max(1, int(spec.size * t.sparsity))
    coeffs, idx, _ = sc.sparsify_np(spec, k)
    differ = sc.check_membership(idx, coeffs, flat, t.freq_coeffs.numpy(), torch.abs(spectrum).numpy().reshape(-1))
    thr = float(torch.abs(t.freq_coeffs).min())
    print(f"  {what}: m {flat.size} (definition {idx.size}), membership differs at {differ}, "
          f"band holds {sc.band_count(torch.abs(spectrum).numpy().reshape(-1), thr)}")


def kept(prefix, t):
    assert max(t.shape) < 2 ** 15
    return {prefix + "indices": t.indices.numpy().astype(np.int16), prefix + "freq_coeffs": t.freq_coeffs.numpy()}


def case(shape, seed):
    name = sc.golden_name(shape, seed)
    print(name)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    act_name, pool_mode = ("relu", "max") if seed == 1 else ("tanh", "avg")
    rec = {"x": x.numpy(), "act_name": np.array(act_name), "pool_mode": np.array(pool_mode)}
    for sparsity in sc.SPARSITIES:
        p = sc.sp_tag(sparsity) + "."
        t, spectrum = reference_sst(lambda: ref_tensor.sst(x, sparsity=sparsity, device="cpu"))
        assert spectrum.dtype == torch.complex64 and tuple(spectrum.shape) == tuple(shape)
        if "spectrum" in rec:
            assert np.array_equal(rec["spectrum"].view(np.uint32), spectrum.numpy().view(np.uint32))
        rec["spectrum"] = spectrum.numpy()
        check_against_definition(t, spectrum, p + "sst")
        rec.update(kept(p, t))
        rec[p + "to_spatial"] = t.to_spatial().numpy()
        rec[p + "normalize"] = ref_ops.spectral_normalize(t).freq_coeffs.numpy()
        a, a_spec = reference_sst(lambda: ref_ops.spectral_activation(t, act_name))
        check_against_definition(a, a_spec, p + "act")
        rec.update(kept(p + "act.", a))
        if len(shape) == 2:
            q, q_spec = reference_sst(lambda: ref_ops.spectral_pool(t, 2, pool_mode))
            check_against_definition(q, q_spec, p + "pool")
            rec.update(kept(p + "pool.", q))
            rec[p + "pool.sparsity"] = np.float64(q.sparsity)
        if tuple(shape) == (32, 32) and seed == 1 and sparsity == 0.2:
            bx = torch.randn(2, 3, 32, generator=torch.Generator().manual_seed(7))
            rec.update({"bsm.x": bx.numpy(), "bsm.block_size": np.int64(16), "bsm.sparsity": np.float64(sparsity),
                        "bsm.out": FrequencyMatMul.block_streaming_matmul(bx, t, block_size=16).numpy()})
    path = os.path.join(HERE, name + ".npz")
    np.savez(path, **rec)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)
                  if f.endswith((".npz", ".npy")) and not f.startswith("Q"))
    assert size <= largest, (size, largest)
    print(f"  {size} bytes")


if __name__ == "__main__":
    for shape in sc.SHAPES:
        for seed in sc.SEEDS:
            case(shape, seed)
