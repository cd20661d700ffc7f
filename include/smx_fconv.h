/* smx_fconv.h -- part of the C ABI of libsmx.so (include/smx.h includes it; the conventions stated there hold: return
 * codes, smx_last_error, streams).  Types stay inside the binding reader's vocabulary: int, long long, size_t, float,
 * void*. */
#ifndef SMX_FCONV_H_
#define SMX_FCONV_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The per-bin channel contraction of the FFT convolutions (fft_tensor/optimized_ops.py:183-187 fast_frequency_conv1d,
 * :247-251 fast_frequency_conv2d: `(x_freq.unsqueeze(1) * w_freq.unsqueeze(0)).sum(dim=2)`): one small complex GEMM per
 * frequency bin.  All tensors complex64, dense, channels innermost, 8-byte aligned; P is a flat count of bins:
 *       forward :  y[b, p, o]  = sum_i x[b, p, i] w[p, i, o]              x (B, P, Ci), w (P, Ci, Co), y (B, P, Co)
 *       backward:  gx[b, p, i] = sum_o gy[b, p, o] conj(w[p, i, o])
 *                  gw[p, i, o] = sum_b conj(x[b, p, i]) gy[b, p, o]       (torch's convention for complex gradients)
 * The (B, Co, Ci, P) product is never formed.  Forward is one launch that reads w once per tile of 8 batch rows (once in
 * all when B <= 8).  Backward is one launch per gradient asked for: gx and gw may each be NULL and are then not computed
 * (gx needs w, gw needs x; the operand the other one needs may be NULL then).  gw with B > 8 re-reads and re-writes gw
 * once per further tile of 8 batch rows, each element by the thread that owns it.  No workspace.
 * max_workgroups: 0 = the launcher's own count; a positive value caps the grid (a workgroup then walks several tiles): a
 * test and tuning knob, the results do not depend on it.
 * 16-byte accesses where an address is 16-byte aligned, 8-byte accesses elsewhere; the arithmetic is the same on both, so
 * every result is a pure function of the inputs (row alignment does not enter): every sum runs in ascending index order,
 * in fp32 FMAs.  No flag words, no atomics on memory, no workgroup waits for another; bitwise reproducible.
 * A zero-sized problem (B, P, Ci or Co == 0) returns SMX_OK and enqueues nothing (with Ci == 0 the caller zero-fills y).
 * Negative sizes, a negative max_workgroups, NULL or misaligned pointers: SMX_ERR_INVALID; sizes beyond
 * smx_bin_contract_supported (P < 2^31, every operand below 2^40 elements): SMX_ERR_UNSUPPORTED.  Nothing is enqueued
 * then, nothing is ever allocated, the host is never synchronised; the calls can be captured in a graph.  The outputs must
 * not overlap the inputs: the caller's promise. */
int smx_bin_contract_supported(int B, long long P, int Ci, int Co);
int smx_bin_contract_forward(const void* x, const void* w, void* y, int B, long long P, int Ci, int Co, int max_workgroups,
                             void* stream);
int smx_bin_contract_backward(const void* x, const void* w, const void* gy, void* gx, void* gw, int B, long long P, int Ci,
                              int Co, int max_workgroups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMX_FCONV_H_ */
