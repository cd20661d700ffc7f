/* smx_freq.h -- part of the C ABI of libsmx.so (include/smx.h includes it; the conventions stated there hold: return
 * codes, smx_last_error, streams, workspaces).  Types stay inside the binding reader's vocabulary: int, long long,
 * size_t, float, void*. */
#ifndef SMX_FREQ_H_
#define SMX_FREQ_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The two native ops of the frequency-domain transformer (fft_tensor/frequency_ops.py:147-185 frequency_attention,
 * :384-401 frequency_layernorm).  Forward only.
 * smx_freq_attention_forward: complex64 q, k, v, out of shape (B, H, N, D), each with ELEMENT strides (complex64 elements)
 *   for its b, h and n axes (x_sb, x_sh, x_sn >= 0) and a contiguous innermost axis, 8-byte aligned:
 *       s[b, h, n] = mean_d |q conj(k)| / temperature,   p = softmax_n(s) (the maximum is subtracted),
 *       out[b, h, n, :] = p[b, h, n] v[b, h, n, :]
 *   so a (B, N, H, hd) tensor is read as its (B, H, N, hd) view and the result can land in (B, N, H hd) layout.  The rows
 *   of `out` must not overlap each other or an input: the caller's promise.  Two launches: one wavefront per row writes
 *   an fp32 score into the workspace (16-byte loads where a row's pairs are 16-byte aligned, D of any size); then every
 *   workgroup of the (tiles of n) x (b h) grid reduces the maximum and the sum of exp over the N scores of its (b, h) in one
 *   fixed order and scales the v rows of its tile.  temperature: finite and not 0.  B H N < 2^31, N <= 2^30.
 *   Workspace: smx_freq_attention_workspace_bytes(B, H, N) (the reserved 64 KiB header, then B H N floats), 256-byte aligned.
 * smx_freq_layernorm_forward: z, out (rows, D) complex64, dense, 16-byte aligned (out may be z).  Per row, m = |z|:
 *       out = (m - mean(m)) / (std(m) + eps) z / |z|,   std unbiased (D = 1: NaN), z / |z| = 1 at z == 0.
 *   One launch, one wavefront per row, the row in registers: D <= SMX_FREQ_LN_MAX_D; a wider row is SMX_ERR_UNSUPPORTED
 *   (the caller composes it).  |z| = sqrt(re^2 + im^2) in fp32: below ~1e-19 it counts as 0, above ~1e19 as inf.
 * No flag words, no atomics on memory, no workgroup waits for another: every result is a pure function of the inputs and
 * of the rows' 16-byte alignment, bitwise reproducible.  A zero-sized problem (B, H, N, D or rows == 0) returns SMX_OK and
 * enqueues nothing.  Negative sizes or strides, NULL pointers, a temperature that is 0 or not finite, a missing, short or
 * unaligned workspace: SMX_ERR_INVALID; sizes beyond the limits above: SMX_ERR_UNSUPPORTED.  Nothing is enqueued then,
 * nothing is ever allocated, the host is never synchronised; the calls can be captured in a graph. */
#define SMX_FREQ_LN_MAX_D 1024
int smx_freq_attention_workspace_bytes(int B, int H, int N, size_t* out);
int smx_freq_attention_forward(const void* q, long long q_sb, long long q_sh, long long q_sn,
                               const void* k, long long k_sb, long long k_sh, long long k_sn,
                               const void* v, long long v_sb, long long v_sh, long long v_sn,
                               void* out, long long o_sb, long long o_sh, long long o_sn, float temperature,
                               void* workspace, size_t workspace_bytes, int B, int H, int N, int D, void* stream);
int smx_freq_layernorm_forward(const void* z, void* out, float eps, long long rows, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMX_FREQ_H_ */
