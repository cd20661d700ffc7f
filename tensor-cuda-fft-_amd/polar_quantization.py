"""Mirror of `fft_tensor.polar_quantization` (reference fft_tensor/polar_quantization.py:15-56): PolarQuantizer, the
magnitude / phase quantiser of a complex64 spectrum into two uint8 planes.  Names, arguments, defaults and attributes are the
reference's; its `test()` function and prints are not mirrored.

On a ROCm device the work is functional.polar_range / polar_quantize / polar_dequantize (csrc/smx_quant.hip): the range is
two launches and ONE host read at the first `quantize` call (the reference reads twice), a quantize is one launch, a
dequantize one launch over LDS tables.  CPU tensors, other dtypes and bit counts above 8 (the reference's own "High-quality"
config has phase_bits = 10, whose codes wrap in the uint8 cast) run the reference's op sequence and give its bits."""
import torch

from . import functional as _fn


class PolarQuantizer:
    def __init__(self, mag_bits=4, phase_bits=8):
        self.mag_bits = mag_bits
        self.phase_bits = phase_bits
        self.mag_levels = 2 ** mag_bits
        self.phase_levels = 2 ** phase_bits
        self.mag_range = None

    def quantize(self, z):
        """complex64 -> (uint8, uint8).  `mag_range`, a tuple of two Python floats (min and max of log2(max(|z|, 1e-9))),
        is fixed by the FIRST call and reused afterwards, as in the reference: later calls do not synchronise, and values
        outside the first tensor's range land on the end codes."""
        if self.mag_range is None:
            lo, hi = _fn.polar_range(z).tolist()
            self.mag_range = (lo, hi)
        return _fn.polar_quantize(z, self.mag_bits, self.phase_bits, self.mag_range)

    def dequantize(self, mag_q, phase_q):
        """(uint8, uint8) -> complex64, with the range `quantize` fixed (TypeError before any, as in the reference)."""
        mag_min, mag_max = self.mag_range
        return _fn.polar_dequantize(mag_q, phase_q, self.mag_bits, self.phase_bits, (mag_min, mag_max))
