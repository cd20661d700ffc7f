/* smx_rowfft.h -- part of the C ABI of libsmx.so (include/smx.h includes it; the conventions stated there and in smx_freq.h
 * hold: return codes, smx_last_error, streams).  Types stay inside the binding reader's vocabulary: int, long long,
 * size_t, float, void*. */
#ifndef SMX_ROWFFT_H_
#define SMX_ROWFFT_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The DFT along the CONTIGUOUS last axis of `rows` dense rows of n points, one launch (csrc/smx_rowfft.hip, k_rowfft).
 * The sequence transform (smx_cfft_ex) takes its vector width from the channel axis; rows of the last axis have no
 * channel axis, and this entry transforms them as they lie: a workgroup holds whole rows in LDS (one row of 4096 points,
 * 2048 rows of 2), so the data is read once and written once.
 *
 * in : (rows, n) complex64, or fp32 with SMX_ROWFFT_REAL_IN;   out: (rows, n) complex64, or fp32 with SMX_ROWFFT_REAL_OUT.
 * For every row r:
 *       a[j] = REAL_IN ? (in_f32[r][j], 0) : in_c64[r][j];        CONJ_IN:  a[j] = conj(a[j])
 *       Y[k] = scale * sum_j a[j] * exp(-2 pi i j k / n)           k = 0..n-1, natural order
 *       CONJ_OUT: Y[k] = conj(Y[k]);                               out[r][k] = REAL_OUT ? Re(Y[k]) : Y[k]
 *   so flags = 0, scale = 1 is torch.fft.fft(dim=-1); CONJ_IN | CONJ_OUT with scale = 1/n is torch.fft.ifft(dim=-1);
 *   CONJ_IN | REAL_OUT with scale = 1/n is ifft(.).real (Re(ifft w) = Re(F conj w) / n); REAL_IN transforms a real tensor
 *   without a complex copy of it.  Arithmetic is fp32; the twiddles are formed in the kernel by sincospif of an exact
 *   binary fraction of a turn, so the call needs no tables, allocates nothing and never synchronises the host; it can be
 *   captured in a graph.
 * n: a power of two from 2 to SMX_ROWFFT_MAX_N (smx_rowfft_supported(n) == 1; no HIP call); every other n:
 *   SMX_ERR_UNSUPPORTED.
 * rows == 0 returns SMX_OK and enqueues nothing.  rows < 0, a negative max_workgroups, unknown flag bits, a NULL pointer,
 *   a pointer that is not 16-byte aligned, a scale that is not finite: SMX_ERR_INVALID.  Every refusal sets smx_last_error
 *   and enqueues nothing.
 * max_workgroups: 0 = the launcher's own count; a positive value caps the grid (a workgroup then walks several groups of
 *   rows): a test and tuning knob, the results do not depend on it.  The grid does not grow with rows past what stays
 *   resident, so rows is bounded by memory alone.
 * In place: out == in is allowed when both sides have the same element type (neither or both of REAL_IN / REAL_OUT): a
 *   workgroup reads its rows whole before it writes any of them, and no other workgroup touches those rows.  Any other
 *   overlap of in and out is the caller's promise not to make.
 * No flag words, no atomics on memory, no workgroup waits for another; only vector stores: a row's result is a pure
 *   function of that row, n, flags and scale -- bitwise reproducible, and independent of rows, of max_workgroups and of
 *   which rows share a workgroup. */
#define SMX_ROWFFT_CONJ_IN  1
#define SMX_ROWFFT_CONJ_OUT 2
#define SMX_ROWFFT_REAL_IN  4
#define SMX_ROWFFT_REAL_OUT 8
#define SMX_ROWFFT_MAX_N    4096
int smx_rowfft_supported(int n);
int smx_rowfft(const void* in, void* out, long long rows, int n, int flags, float scale,
               int max_workgroups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMX_ROWFFT_H_ */
