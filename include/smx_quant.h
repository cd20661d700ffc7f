/* smx_quant.h -- part of the C ABI of libsmx.so (include/smx.h includes it; the conventions stated there and in smx_freq.h
 * hold: return codes, smx_last_error, streams, workspaces).  Types stay inside the binding reader's vocabulary: int,
 * long long, size_t, float, void*. */
#ifndef SMX_QUANT_H_
#define SMX_QUANT_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The codecs of the compressed spectra: the polar quantiser (fft_tensor/polar_quantization.py:23-56, PolarQuantizer) and
 * the 8-bit logarithmic one (fft_tensor/zero_materialize.py:470-568, LogarithmicQuantizer), each as ONE pass over n dense
 * elements.  z: complex64, 8-byte aligned; x: fp32, 4-byte aligned; every code plane: uint8 at ANY byte address.
 *
 * Polar, with Lm = 2^mag_bits - 1, Lp = 2^phase_bits - 1 (bit counts 1..8) and lg(z) = log2(max(|z|, 1e-9)):
 *       u = (lg(z) - mag_min) / (mag_max - mag_min + 1e-9) * Lm        mag_q   = clamp(rint(u), 0, Lm)
 *       v = (atan2(im, re) + pi) / (2 pi) * Lp                         phase_q = clamp(rint(v), 0, Lp)
 *       dequantize:  z = 2^(mag_q / Lm * (mag_max - mag_min) + mag_min) * (cos, sin)(phase_q / Lp * 2 pi - pi)
 *   rint rounds half to even (torch.round).  |z|^2 is formed as re^2 + im^2 in fp32 and lg as half its log2: a |z| below
 *   about 1e-19 counts as 0 (inside the 1e-9 clamp: no difference), one above about 1e19 as inf, which lands on the top
 *   code -- the correct one.  A NaN element gives code 0 and does not enter the range.  The range arrives as two host
 *   floats (smx_polar_range computes it on the device; the caller reads it back once and may reuse it).
 *   smx_polar_range: out2 = two fp32 on the device, (min, max) over the elements of lg(z).  Two launches: per-workgroup
 *   (min, max) pairs of re^2 + im^2 into the workspace, then a one-workgroup join that applies lg to the two ends (log2 is
 *   monotone) -- with the function smx_polar_quantize applies per element, so an input of one repeated magnitude has
 *   u == 0 exactly.  Workspace: smx_polar_range_workspace_bytes(n), 256-byte aligned.
 *   smx_polar_dequantize: each workgroup first builds the 256-entry tables of magnitudes and unit vectors in LDS (a byte
 *   above the top code extrapolates the formula, as the reference's arithmetic does), then streams without a
 *   transcendental.  One launch, as smx_polar_quantize.
 * log8 (fp32 <-> uint8):
 *       e = (x >= 0) << 7 | trunc(clamp((log2(|x| + 1e-8) + 8) / 16 * 127, 0, 127))      (+-0.0 both carry the sign bit)
 *       x = (bit 7 ? +1 : -1) * 2^((e & 127) / 127 * 16 - 8)                               (a 256-entry LDS table)
 *   A NaN encodes to 0.  The _c64 entries run the codec on the real and imaginary parts of a complex64 tensor in one
 *   pass over the interleaved data (LogarithmicQuantizer.compress_sparse_freq / decompress_sparse_freq).
 *
 * The wide side is moved in 16-byte accesses from its first 16-byte address on (elements before it, at most 1 complex or 3
 * fp32, and fewer than 4 at the end go one by one); a plane moves 4 bytes per lane, as one dword where that address is
 * 4-byte aligned.  max_workgroups: 0 = the launcher's own count; a positive value caps the grid (a workgroup then walks
 * several tiles): a test and tuning knob, the results do not depend on it.
 * No flag words, no atomics on memory, no workgroup waits for another; only vector stores: every result is a pure function
 * of the inputs, bitwise reproducible.  n == 0 returns SMX_OK and enqueues nothing (the workspace query answers 0).
 * n < 0, a negative max_workgroups, NULL or misaligned pointers, bit counts outside 1..8, a missing, short or unaligned
 * workspace: SMX_ERR_INVALID.  Nothing is enqueued then, nothing is ever allocated, the host is never synchronised; the
 * calls can be captured in a graph.  Outputs must not overlap inputs: the caller's promise. */
int smx_polar_range_workspace_bytes(long long n, size_t* out);
int smx_polar_range(const void* z, long long n, void* out2, void* workspace, size_t workspace_bytes, int max_workgroups,
                    void* stream);
int smx_polar_quantize(const void* z, void* mag_q, void* phase_q, long long n, int mag_bits, int phase_bits, float mag_min,
                       float mag_max, int max_workgroups, void* stream);
int smx_polar_dequantize(const void* mag_q, const void* phase_q, void* z, long long n, int mag_bits, int phase_bits,
                         float mag_min, float mag_max, int max_workgroups, void* stream);
int smx_log8_encode(const void* x, void* out, long long n, int max_workgroups, void* stream);
int smx_log8_decode(const void* e, void* x, long long n, int max_workgroups, void* stream);
int smx_log8_encode_c64(const void* z, void* re_q, void* im_q, long long n, int max_workgroups, void* stream);
int smx_log8_decode_c64(const void* re_q, const void* im_q, void* z, long long n, int max_workgroups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMX_QUANT_H_ */
