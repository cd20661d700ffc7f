/* smx.h -- C ABI of the MI355X spectral-mixing library (libsmx.so).
 *
 * The reference (fricker2025-star/Tensor-Cuda-FFT-) is pure PyTorch and has NO FFI for this path;
 * its boundary is the Python nn.Module API.  These entry points are what a native binding of
 * that API binds to; each one names the reference lines it replaces (paths relative to the
 * reference root).  See INTEGRATION.md for the reference-side ctypes stub.
 *
 * Conventions
 *  - Every buffer is DEVICE memory owned by the caller (fp32, contiguous, row-major).
 *    Complex tensors are interleaved (re,im) fp32 pairs == torch.complex64.
 *  - x, y, g, grad_x : (B, N, D).  w_re, w_im : (D, F).  bias : (D).
 *    k = min(F, N/2) kept bins (integer division).  Spectra xk/gk : (B, k, D) complex.
 *  - All work is enqueued on `stream` (a hipStream_t; NULL = default stream).  No host sync,
 *    except the one-time twiddle-table upload the first time a given N is seen on a device.
 *    That upload is REFUSED (SMX_ERR_UNSUPPORTED, nothing enqueued) while `stream` is being
 *    captured into a hipGraph: call smx_prepare(N), or run one eager call of the shape, first.
 *    The table cache holds "table_cache_entries" (default 256) sequence lengths per process;
 *    beyond that the least recently used ones OF THE CALLING DEVICE that no call in flight is using are freed
 *    after a device synchronise (smx_tables_epoch() changes).
 *  - Return value: 0 on success, negative SMX_ERR_* otherwise; text via smx_last_error()
 *    (thread-local).  Nothing throws across this boundary.
 *  - Thread-safe; re-entrant across streams and devices (uses the calling thread's current device).
 */
#ifndef SMX_H_
#define SMX_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMX_VERSION 303            /* 0.3.3: smx_spectral_gate_* (0.3.2: smx_diag_clock; conv / cfft workspaces behind the reserved 64 KiB header) */

#define SMX_OK 0
#define SMX_ERR_INVALID (-1)       /* bad shape / null pointer / misaligned buffer */
#define SMX_ERR_UNSUPPORTED (-2)
#define SMX_ERR_HIP (-3)           /* a HIP runtime call failed; see smx_last_error() */
#define SMX_ERR_WORKSPACE (-4)     /* workspace too small; see smx_workspace_bytes() */

/* which kernels a shape is routed to */
#define SMX_PATH_DECIMATED 1       /* N % 256 == 0, D even, k <= 512: fused Stockham radix-16x16 */
#define SMX_PATH_DIRECT 2          /* everything else: pruned DFT as matrix products, O(N k) per column */
#define SMX_PATH_DECIM16 3         /* n_fft % 16 == 0 (not % 256), D even, k <= 256 (rows <= n_fft zero-padded): one
                                      16-point transform per residue + O(N k / 16) accumulation, x read once,
                                      y written once (k_fused16; fused dropout and every phase split included);
                                      synthesis alone runs the DFT products of SMX_PATH_DIRECT, row_scale is refused */

typedef struct smx_plan {
  int path;        /* SMX_PATH_*                                                      */
  int k;           /* kept bins                                                       */
  int L;           /* decimation factor N/256            (decimated path)             */
  int bands;       /* 1: k <= 128, 2: k <= 256, 4: k > 256 (decimated path)           */
  int nsplit;      /* residue chunks; 1 = single fused launch per direction           */
  int workgroups;  /* workgroups of the transform launch                              */
  int groups;      /* band groups of 512 bins: 1 unless k > 512 (one launch per group) */
} smx_plan;

int smx_version(void);
const char* smx_last_error(void);

/* Tuning knobs, process-wide DEFAULTS: "nsplit" (0 = auto), "placement" (workgroup -> tile map: 0 b-major,
 * 1 rotated residues, 2 XCD-aware = default, 3 | a << 8 | b << 16 = XCD-aware with the residue rotation
 * (a l2 + b d_tile) mod L, used by tools/rot_scan.py), "round" (workgroups per launch of the streaming
 * kernels, default 512 = one resident round; 0 = a single launch), "force_direct" (0/1), "full8", "fourstep",
 * "fs_bgroups", "tiled_dft", "decim16", "conv1", "st_plain" (A/B switches of DESIGN.md), "table_cache_entries" (twiddle-table cache bound).
 * "fold_gradw" is RETIRED: still accepted (and counted by smx_options_epoch), without effect on any plan, workspace or result.
 * "st_layout_fwd" / "st_layout_bwd" ("st_layout" sets both): WHICH of a thread's 16 rows per tile are the st_plain
 * write-back rows of the buffer-addressed streaming stores in the forward / backward launches: -2 (default) by the library's
 * rule (4 on the single-launch plan up to 320 MiB of output, else -1: DESIGN.md section 4.6); -1 the first
 * ones, one contiguous block per batch row; 0 every (16 / st_plain)-th row; 1 .. 4 the same rotated per tile by the
 * residue r, by r >> 2, by the wave index, by wave index + r.  Process-wide only -- not a
 * member of smx_options, which cannot grow -- and without effect on any result or workspace layout. */
int smx_set_option(const char* name, int value);

/* The same knobs as an argument of the calling context: every call THIS THREAD makes between
 * smx_options_push(opts) and the matching smx_options_pop() plans with *opts instead of the process-wide
 * defaults (nestable, 8 deep).  Two users of one process can therefore run different plans, and a plan query /
 * workspace size / forward / backward sequence made under one push is consistent by construction.
 * smx_options_default fills *out with the current defaults (start from it, change what you need).
 * smx_options_epoch() changes whenever a process-wide default changes: anything memoised per shape outside a
 * push (plan, workspace size) is valid for one epoch.  smx_tables_epoch() changes whenever twiddle tables are
 * evicted from the cache: a shape "prepared" for stream capture before that may need smx_prepare again. */
typedef struct smx_options {
  int nsplit, placement, round, force_direct, full8, fourstep, fs_bgroups;
  int fold_gradw;   /* RETIRED, no effect: the parameter gradients are always reduced by a launch of their own
                       (k_gradw_slab).  The field keeps its place because the layout of this struct is ABI. */
  int decim16;      /* 1 (default): SMX_PATH_DECIM16 is used where it applies; 0: DFT products (A/B, tests) */
  int conv1;        /* 1 (default): smx_conv_* run ONE launch per direction for n_fft = 512, 1024, 2048
                       (k_conv1) from 48 (batch row, 32-channel tile) items on -- as 256-thread
                       workgroups on 16 channels up to 768 items, 512-thread workgroups on 32 channels above;
                       2 / 3: wherever the shape allows it with 32- / 16-channel workgroups; 0: the three launches
                       of the four-step form (A/B, tests).  The layout of x_spectra differs between the forms:
                       forward and backward of one call pair must run under the same value */
  int st_plain;     /* rows (of the 16 a thread writes per tile) that the streaming kernels store with the DEFAULT
                       write-back policy instead of the streaming hint: -1 (default) = by the size of the output
                       tensor, about 64 MiB of it (4 rows up to 320 MiB, 2 up to 768 MiB, 1 up to 1.5 GiB, else 0);
                       0, 1, 2, 4 = that many (A/B).  DESIGN.md section 4, round 4 */
} smx_options;
int smx_options_default(smx_options* out);
int smx_options_push(const smx_options* opts);
int smx_options_pop(void);
unsigned long long smx_options_epoch(void);
unsigned long long smx_tables_epoch(void);

/* Compile-time switches of this binary that change what the kernels compute ("" for the shipped build).
 * A name starting with SMX_AB_ marks a timing-ablation build that returns wrong results by design. */
const char* smx_build_flags(void);

/* Diagnostic (no reference counterpart): the shader clock the chip sustains right now.  One wavefront reads
 * s_memtime (core-clock ticks) and s_memrealtime (the constant 100 MHz counter) around `spin` dependent FMAs and
 * stores both differences: out2[0] / out2[1] * 0.1 = GHz.  bench.py enqueues it right behind its timed region and
 * stamps the figure on its line, so a slow box can be told from a slow build (the fused launches follow the clock:
 * DESIGN.md section 4).  out2: two 64-bit words in device memory. */
int smx_diag_clock(unsigned long long* out2, int spin, void* stream);

int smx_plan_query(int B, int N, int D, int F, smx_plan* out);
int smx_workspace_bytes(int B, int N, int D, int F, size_t* out);
int smx_prepare(int N);

/* y = real(ifft(pad_k(W .* fft(x)[:k]))) + bias
 *   replaces SpectralMixingLayer.forward, fft_tensor/spectral_layers.py:88-116.
 *   bias may be NULL.  xk_save (B,k,D) complex may be NULL; when given it receives fft(x)[:, :k, :]
 *   (what backward needs -- the reference keeps the whole x_freq alive instead, :88).
 *   conj_w != 0 multiplies by conj(W): with bias == NULL that is grad_x of the same layer. */
int smx_forward(const float* x, const float* w_re, const float* w_im, const float* bias, float* y,
                float* xk_save, void* workspace, size_t workspace_bytes, int B, int N, int D, int F,
                int conj_w, void* stream);

/* Autograd backward of the lines above for upstream gradient g:
 *   grad_x = real(ifft(pad_k(conj(W) .* fft(g)[:k]))),
 *   grad_w_real[d,f] = Re P, grad_w_imag[d,f] = -Im P, P[f,d] = (1/N) sum_b X conj(G)   (f < k, else 0),
 *   grad_bias[d] = sum_{b,n} g.
 * phases (bit mask, SMX_PHASE_ALL = one fused launch when the plan allows):
 *   SMX_PHASE_SPECTRUM  transform g, filter, per-batch-row products X conj(G)   (into the workspace)
 *   SMX_PHASE_INVERSE   inverse transform to grad_x                             (needs SPECTRUM first)
 *   SMX_PHASE_PARAMS    reduce the products to gw_re / gw_im / gbias           (needs SPECTRUM first)
 *   Separate calls on the same workspace let a multi-GPU caller run PARAMS + the all-reduce of the
 *   parameter gradients on a side stream while INVERSE runs on the main one.
 * gw_re / gw_im / gbias may be NULL together (input gradient only; PARAMS is then a no-op, but pass
 * them to the SPECTRUM call too when PARAMS will follow). */
#define SMX_PHASE_SPECTRUM 1
#define SMX_PHASE_INVERSE 2
#define SMX_PHASE_PARAMS 4
#define SMX_PHASE_ALL 7
/* SMX_PHASE_SYNC_CLEAN: accepted in `phases` and IGNORED (it vouched for flag words of the retired option fold_gradw).
 * It selects no phase: `phases` = 8 alone is refused like 0.  The first 64 KiB of every workspace layout, once those
 * flag words, stay reserved: nothing reads or writes them. */
#define SMX_PHASE_SYNC_CLEAN 8
int smx_backward(const float* g, const float* xk, const float* w_re, const float* w_im,
                 float* grad_x, float* gw_re, float* gw_im, float* gbias, void* workspace,
                 size_t workspace_bytes, int B, int N, int D, int F, int phases, void* stream);

/* xk = fft(x, dim=1)[:, :k, :]   (spectral_layers.py:88 restricted to the bins :94-101 keep) */
int smx_spectrum(const float* x, float* xk, void* workspace, size_t workspace_bytes, int B, int N,
                 int D, int F, void* stream);

/* Parameter gradients from two saved spectra (same formulas as smx_backward). */
int smx_grad_w(const float* xk, const float* gk, float* gw_re, float* gw_im, float* gbias, int B,
               int N, int D, int F, void* stream);

/* WirtingerSpectralFilter.forward, fft_tensor/wirtinger_ops.py:170-203:
 *   out[b,n,d] = n < k ? x_freq[b,n,d] * (w_re + i w_im)[d,n] : 0      (complex (B,N,D) in/out)
 *   conj_w != 0 gives the filter's grad_x (wirtinger_ops.py:71). */
int smx_wfilter_forward(const float* x_freq, const float* w_re, const float* w_im, float* out, int B,
                        int N, int D, int F, int conj_w, void* stream);
/* grad of the filter weights: sum_b g * conj(x) on bins < k (wirtinger_ops.py:77-80), split into
 * the gradients of ComplexParameter.real / .imag (wirtinger_ops.py:132-134); columns >= k are zero. */
int smx_wfilter_grad_w(const float* x_freq, const float* g_freq, float* gw_re, float* gw_im, int B,
                       int N, int D, int F, void* stream);

/* WirtingerGradient, fft_tensor/wirtinger_ops.py:45-50 and :67-82, for w broadcast over the
 * leading dimension: x (batch, inner) complex, w (inner) complex.
 *   smx_cmul:        out = x * w          (conj_w: x * conj(w)  == grad_x)
 *   smx_cmul_grad_w: gw  = sum_batch g * conj(x) */
int smx_cmul(const float* x, const float* w, float* out, long long batch, long long inner,
             int conj_w, void* stream);
int smx_cmul_grad_w(const float* x, const float* g, float* gw, long long batch, long long inner,
                    void* stream);

/* ---- general shapes: zero-padded rows, explicit bin count, Nyquist bin ------------------------------
 * The same transform for the callers either side of the layer:
 *   y[:, :rows] = real(ifft_{n_fft}( pad_k( W .* fft_{n_fft}(zero-pad(x))[:k] ) ))[:, :rows] + bias
 * x, y, g, grad_x : (B, rows, D), rows <= n_fft -- rows beyond `rows` are zeros on the way in and are
 * not written on the way out: the causal FFT convolution of fft_lm.FixedSpectralBlock (reference
 * fft_lm/train_fixed_full.py:507-519 zero-pad to a power of two, :553-555 crop).
 * k <= min(F, n_fft/2 + 1) kept bins, spectra (B, k, D); k = n_fft/2 + 1 is the full one-sided spectrum
 * incl. the Nyquist bin, of which -- as of DC -- only Re(W X) reaches the real output.  The convention
 * stays the layer's (one-sided spectrum, real part: bins 1 .. n_fft/2 - 1 count once); torch.fft.irfft
 * semantics (reference spectral_enhancements.py:164, train_fixed_full.py:553) = the same call with W
 * doubled on those bins, which the Python callers do (functional.hermitian_weights).
 * With rows = n_fft and k = min(F, n_fft/2) these are smx_forward / smx_backward / smx_spectrum (no
 * fused dropout here).  filter_pack as below. */
typedef struct smx_shape {
  int B;        /* batch                                    */
  int rows;     /* rows of x / y / g / grad_x               */
  int D;        /* channels                                 */
  int F;        /* columns of w_re / w_im (D, F)            */
  int n_fft;    /* transform length, >= rows                */
  int k;        /* kept bins, <= min(F, n_fft/2 + 1)        */
} smx_shape;
int smx_plan_query_ex(const smx_shape* shape, smx_plan* out);
int smx_workspace_bytes_ex(const smx_shape* shape, size_t* out);
/* row_scale (may be NULL): (B, D) real factors, W_eff[b,d,f] = W[d,f] * row_scale[b,d] -- the context gate
 * of FixedSpectralBlock (train_fixed_full.py:532-536: g_ctx multiplies every bin of a (batch, channel)
 * column) applied inside the filter stage instead of as a pass over y.  Backward given the same row_scale
 * returns gw_re / gw_im with the factor included and, in grad_row_scale (B, D; may be NULL),
 * d/d row_scale = sum_n g * y0 with y0 the unscaled output.  Available where smx_row_scale_supported()
 * says so (every decimated plan except the band groups); SMX_ERR_UNSUPPORTED otherwise. */
int smx_row_scale_supported(const smx_shape* shape);
int smx_forward_ex(const smx_shape* shape, const float* x, const float* w_re, const float* w_im,
                   const float* bias, float* y, float* xk_save, void* workspace, size_t workspace_bytes,
                   int conj_w, float* filter_pack, const float* row_scale, void* stream);
int smx_backward_ex(const smx_shape* shape, const float* g, const float* xk, const float* w_re,
                    const float* w_im, float* grad_x, float* gw_re, float* gw_im, float* gbias,
                    void* workspace, size_t workspace_bytes, int phases, const float* filter_pack,
                    const float* row_scale, float* grad_row_scale, void* stream);
/* xk = rfft(zero-pad(x), n_fft)[:, :k, :]   (reference train_fixed_full.py:515-519,
 * spectral_enhancements.py:147, :237; frequency_ops.py:201 via the channel-pair packing) */
int smx_spectrum_ex(const smx_shape* shape, const float* x, float* xk, void* workspace,
                    size_t workspace_bytes, void* stream);

/* torch.fft.fft(z, dim=1) of a COMPLEX (B, rows, D/2) tensor handed over as real (B, rows, D): a channel pair
 * is one complex channel, so the packed spectrum the kernels form is the answer -- out (B, n_fft, D) real =
 * (B, n_fft, D/2) complex, every bin (FrequencyAttention.fnet_attention, fft_tensor/frequency_ops.py:188-204).
 * n_fft = 256 L with L in {2, 4, 5..32, 36..64 step 4, 72..128 step 8, 144..256 step 16} and even D (shape->F, k are ignored; workspace from
 * smx_cfft_workspace_bytes): SMX_ERR_UNSUPPORTED otherwise -- compose it from smx_spectrum_ex there
 * (Z[f] = A[f] + i B[f], Z[n_fft - f] = conj A[f] + i conj B[f]), as functional.seq_fft does. */
int smx_cfft_workspace_bytes(const smx_shape* shape, size_t* out);
int smx_cfft_ex(const smx_shape* shape, const float* z, float* out, void* workspace, size_t workspace_bytes,
                void* stream);

/* The differentiable transform pair of the blocks that work ON the spectrum between the two transforms
 * (reference fft_lm/frequency_native.py:316-317 / :355-356 FrequencyNativeBlock, fft_lm/bicameral.py:170-171 /
 * :203-204 BicameralBlock, fft_tensor/spectral_enhancements.py:152 / :166): with theta = 2 pi f n / n_fft and
 * c_f = 2 for 0 < f < n_fft/2 when `hermitian`, else 1,
 *   smx_rfft_ex   spec[b, f, d] = scale * c_f * sum_{n < rows} x[b, n, d] e^{-i theta}              f < k
 *   smx_irfft_ex  y[b, n, d]    = scale * sum_{f < k} c_f * Re( spec[b, f, d] e^{+i theta} )        n < rows
 * (the imaginary parts of the DC and Nyquist rows do not reach y, as in torch.fft.irfft).
 *   torch.fft.rfft(x, n_fft, dim=1)[:, :k]      = smx_rfft_ex(scale 1, hermitian 0)  (= smx_spectrum_ex)
 *   torch.fft.irfft(spec, n_fft, dim=1)[:, :rows] = smx_irfft_ex(scale 1/n_fft, hermitian 1), k = n_fft/2 + 1
 *   backward of rfft:  grad_x = smx_irfft_ex(grad_spec, scale 1, hermitian 0)
 *   backward of irfft: grad_spec = smx_rfft_ex(grad_y, scale 1/n_fft, hermitian 1)
 * spec is (B, k, D) complex64 interleaved, 16-byte aligned; workspace as smx_workspace_bytes_ex(shape).
 * shape.F is only required to be >= k. */
int smx_rfft_ex(const smx_shape* shape, const float* x, float* spec, float scale, int hermitian,
                void* workspace, size_t workspace_bytes, void* stream);
int smx_irfft_ex(const smx_shape* shape, const float* spec, float* y, float scale, int hermitian,
                 void* workspace, size_t workspace_bytes, void* stream);

/* The causal FFT convolution of fft_lm.FixedSpectralBlock with its own kernels (reference
 * fft_lm/train_fixed_full.py:507-555; twin backward fft_lm/frequency_native.py:107-121):
 *   y[b, n, c] = row_scale[b, c] * irfft( rfft(zero-pad(x[b, :, c]), n_fft) * H, n_fft )[n],   n < rows
 * H (n_fft/2 + 1 complex: h_re, h_im) is shared by every channel -- kernel spectrum x frequency gate x cutoff
 * mask -- and row_scale (B, D; may be NULL) carries gain x context gate.  A real kernel convolves the packed
 * channel pair as it convolves each channel, so the packed spectrum is multiplied by the Hermitian extension of
 * H directly: no (D, F) filter, no unpack, no one-sided spectrum or gradient slab.
 * forward writes the tile spectra of x into x_spectra (save_bytes of smx_conv_workspace_bytes; may be NULL when
 * no backward follows); backward needs them and returns
 *   grad_x, grad_row_scale (B, D; may be NULL) = sum_n g * y0 (y0 = output before row_scale), and
 *   grad_h_re / grad_h_im (n_fft/2 + 1 each; may be NULL together) = dL/dRe H, dL/dIm H: with
 *   P[f] = sum over (b, channel pairs) of Zg[f] (sigma conj Zx[f] + delta Zx[-f]) the Hermitian part
 *   Q[f] = (P[f] + conj P[n_fft - f]) / 2 is sum_c s_c conj(X_c) G_c and dL/dH[f] = c_f Q[f] / n_fft, c_f = 2 (1 at
 *   DC and Nyquist, whose imaginary parts do not reach the output and get gradient 0).
 * n_fft = 512, 1024, 2048 (fft_lm's default: seq_len 1024 + 128 taps) run ONE launch per direction (k_conv1, option
 * "conv1"): with rows <= n_fft / 2 the n_fft-point spectrum splits by parity of the bin into two half-length transforms
 * of the same rows, and one workgroup holds both; more rows are first folded onto the lower half (x[n] +/- x[n + n_fft/2]
 * at the load, two output rows per value at the store).  x is read once, y written once; x_spectra then holds the packed
 * spectrum in that kernel's own layout (same save_bytes).  Other lengths: three launches through a workspace.
 * Shapes: shape->{B, rows, D, n_fft}; F and k are ignored.  Available for n_fft = 512 ... 65536 (powers
 * of two) with even D (smx_conv_supported); other lengths go through smx_forward_ex with W[c, f] = c_f H[f] gain[c] and
 * row_scale. */
int smx_conv_supported(const smx_shape* shape);
int smx_conv_workspace_bytes(const smx_shape* shape, size_t* workspace_bytes, size_t* save_bytes);
int smx_conv_forward(const smx_shape* shape, const float* x, const float* h_re, const float* h_im,
                     const float* row_scale, float* y, float* x_spectra, void* workspace,
                     size_t workspace_bytes, void* stream);
int smx_conv_backward(const smx_shape* shape, const float* g, const float* x_spectra, const float* h_re,
                      const float* h_im, const float* row_scale, float* grad_x, float* grad_h_re,
                      float* grad_h_im, float* grad_row_scale, void* workspace, size_t workspace_bytes,
                      void* stream);
/* 2-byte activations of the convolution: smx_conv_forward_io / smx_conv_backward_io are smx_conv_forward /
 * smx_conv_backward with x, y, g, grad_x in the element type `io` (SMX_IO_F32: exactly the f32 entries; SMX_IO_BF16,
 * SMX_IO_F16, defined below).  Everything else keeps its f32 type and layout: h_re, h_im, row_scale, their gradients,
 * x_spectra (same save_bytes) and the workspace (same size).  Arithmetic is f32: the input widens exactly on load,
 * y / grad_x are rounded once at the store, to nearest even (a NaN stays a NaN, fp16 overflow goes to +-inf) -- each
 * output equals the f32 entry's output on the widened input rounded to `io`, bit for bit; x_spectra and the gradients
 * of h and row_scale equal the f32 entry's, bit for bit.
 * Native 2-byte rows exist on the single-launch plan only (n_fft <= 2048, option "conv1" taking the shape:
 * smx_conv_io_supported == 1).  Any other plan returns SMX_ERR_UNSUPPORTED: the caller widens the input itself and
 * calls the f32 entry.  Pointers: x / y / g / grad_x 4-byte aligned for a 2-byte `io` (8 for SMX_IO_F32).
 * Replaces: reference fft_lm/train_fixed_full.py:515-555 (rfft, response product, irfft, crop) and its autograd
 * backward in bf16 / fp16 -- which the reference's torch.fft refuses (bf16) or runs in complex32 (fp16). */
int smx_conv_io_supported(const smx_shape* shape, int io);
int smx_conv_forward_io(const smx_shape* shape, const void* x, const float* h_re, const float* h_im,
                        const float* row_scale, void* y, float* x_spectra, void* workspace,
                        size_t workspace_bytes, int io, void* stream);
int smx_conv_backward_io(const smx_shape* shape, const void* g, const float* x_spectra, const float* h_re,
                         const float* h_im, const float* row_scale, void* grad_x, float* grad_h_re,
                         float* grad_h_im, float* grad_row_scale, void* workspace, size_t workspace_bytes,
                         int io, void* stream);

/* The response the block hands to smx_conv_*, in one launch (reference fft_lm/train_fixed_full.py:511-513 k_freq,
 * :529 frequency gate, :540-551 cutoff mask):
 *   H[f] = rfft(zero-pad(kernel[0 .. taps), n_fft))[f] * sigmoid(gate_logits[f]) * mask[f],   f <= n_fft / 2
 * gate_logits (at least n_fft/2 + 1 entries) and mask (n_fft/2 + 1) may each be NULL (= factor 1).
 * backward: from grad_h_re / grad_h_im (n_fft/2 + 1, e.g. smx_conv_backward's) the gradients of the taps
 * (grad_kernel, taps; may be NULL) and of the logits (grad_gate_logits, n_logits entries, zero from n_fft/2 + 1 on;
 * may be NULL).  Deterministic (fixed summation order). */
int smx_conv_response(int n_fft, int taps, const float* kernel, const float* gate_logits, const float* mask,
                      float* h_re, float* h_im, void* stream);
int smx_conv_response_backward(int n_fft, int taps, int n_logits, const float* kernel, const float* gate_logits,
                               const float* mask, const float* grad_h_re, const float* grad_h_im, float* grad_kernel,
                               float* grad_gate_logits, void* stream);

/* The filter of PhaseAwareSpectralMixing (reference fft_tensor/spectral_enhancements.py:147-164: magnitude * m[d],
 * phase + p[d] on every bin, then irfft) as the (D, k) arrays smx_forward_ex takes:
 *   W[d, f] = c_f * magnitude[d] * exp(i * phase[d]),  f < k <= n_fft/2 + 1;  c_f = 2, 1 at DC and at the Nyquist bin of
 *   an even n_fft (torch.fft.irfft's weights).
 * backward: grad_magnitude[d] = sum_f c_f (gW_re cos p + gW_im sin p), grad_phase[d] = m[d] sum_f c_f (gW_im cos p -
 * gW_re sin p) from the (D, row_pitch) gradient arrays of smx_backward_ex (either output may be NULL). */
int smx_phase_filter(const float* magnitude, const float* phase, int D, int k, int n_fft, float* w_re, float* w_im,
                     void* stream);
int smx_phase_filter_backward(const float* magnitude, const float* phase, const float* grad_w_re, const float* grad_w_im,
                              int D, int k, int n_fft, int row_pitch, float* grad_magnitude, float* grad_phase,
                              void* stream);

/* First half of SpectralMLPBlock.forward, fft_tensor/spectral_layers.py:185 (with :154-158, :162):
 *   y = x + SpectralMixingLayer(LayerNorm(x; ln_w, ln_b, eps))            (dropout inactive)
 * ln_w / ln_b (D) may be NULL (elementwise_affine=False).  ln_stats (B,N,2) receives (mean, rstd) per
 * row and xk_save (B,k,D) complex the spectrum of the normalised input; backward needs both plus x.
 * On the decimated single-launch plan the normalisation is applied while x is loaded and x is added
 * while y is stored (HBM traffic 16 B/sample instead of 28); other plans run the same arithmetic
 * unfused.  y must not alias x.  smx_block_supported(D) == 0 -> SMX_ERR_UNSUPPORTED. */
int smx_block_supported(int D);
int smx_block_forward(const float* x, const float* ln_w, const float* ln_b, float eps,
                      const float* w_re, const float* w_im, const float* bias, float* y,
                      float* xk_save, float* ln_stats, void* workspace, size_t workspace_bytes,
                      int B, int N, int D, int F, void* stream);

/* Autograd backward of smx_block_forward for upstream gradient g:
 *   grad_h = smx_backward(g)            (filter gradients as there, from xk = spectrum of LayerNorm(x))
 *   grad_x = g + LayerNorm'(grad_h)     (torch.nn.LayerNorm backward; written over grad_h in place)
 *   g_ln_w[d] = sum_{b,n} grad_h * xhat,  g_ln_b[d] = sum_{b,n} grad_h     (either may be NULL)
 * phases as in smx_backward; the LayerNorm backward (grad_x, g_ln_w, g_ln_b) belongs to
 * SMX_PHASE_INVERSE. */
int smx_block_backward(const float* g, const float* x, const float* ln_stats, const float* ln_w,
                       const float* xk, const float* w_re, const float* w_im, float* grad_x,
                       float* g_ln_w, float* g_ln_b, float* gw_re, float* gw_im, float* gbias,
                       void* workspace, size_t workspace_bytes, int B, int N, int D, int F,
                       int phases, void* stream);

/* Training-mode dropout of SpectralMixingLayer.forward (nn.Dropout on y + bias, spectral_layers.py:68, :118)
 * fused into the same launches: the "_dropout" twins take the drop probability p in [0, 1) (quantised to
 * 1/65536; p = 0 is the plain call) and rng_state, a DEVICE pointer to two 64-bit words (seed, call
 * counter).  The mask is a counter-based function of (rng_state, batch row, element index): the forward
 * call applies it to y (after the bias, before the block's residual) scaled by 1/(1-p), the backward call
 * given the SAME two words applies it to g.  It is this library's generator, not torch's: same
 * distribution, different bits.  smx_rng_next copies `state` to `saved` (hand `saved` to forward and
 * backward) and advances the counter, all on the device, so a captured hipGraph draws a new mask at
 * every replay.  With more than 512 kept bins the same mask is one more pass inside the call instead of part of a tile
 * store / load: forward on y; backward stages the masked g in grad_x (four-step and eight-band plans: grad_x must then
 * be given, and the eight-band plan wants the SPECTRUM and INVERSE phases in one call) or in a (B, N, D) row copy the
 * workspace holds (band-group plan, smx_plan.groups > 1 -- which for that reason cannot transform in place).
 * Zero-padded rows (smx_*_ex with rows < n_fft) refuse p > 0 with SMX_ERR_UNSUPPORTED.
 * filter_pack (may be NULL): a (k, D) complex64 device buffer, k = min(F, N/2), 16-byte aligned.  The
 * forward call fills it with the filter in the layout its kernels read (pack[f, d] = W[d, f]; without
 * it that copy goes to the workspace); the backward call given the same buffer -- and unchanged weights
 * -- skips its own packing launch.  A forward call may skip it too (constant weights, e.g. inference):
 * OR SMX_FILTER_PACK_READY into conj_w and pass the buffer an earlier forward call filled.  (Two cases
 * never pack and leave the buffer untouched: problems below 8 Mi samples -- the launch would cost more
 * than it saves -- and one band (k <= 128), where every workgroup stages its own 32-channel slice of
 * (D, F) through LDS.) */
#define SMX_FILTER_PACK_READY 2
int smx_rng_next(void* state, void* saved, void* stream);
int smx_forward_dropout(const float* x, const float* w_re, const float* w_im, const float* bias,
                        float* y, float* xk_save, void* workspace, size_t workspace_bytes, int B,
                        int N, int D, int F, int conj_w, float dropout_p, const void* rng_state,
                        float* filter_pack, void* stream);
int smx_backward_dropout(const float* g, const float* xk, const float* w_re, const float* w_im,
                         float* grad_x, float* gw_re, float* gw_im, float* gbias, void* workspace,
                         size_t workspace_bytes, int B, int N, int D, int F, int phases,
                         float dropout_p, const void* rng_state, const float* filter_pack,
                         void* stream);
/* ---- 2-byte activations ------------------------------------------------------------------------------------------
 * smx_forward_io / smx_backward_io: smx_forward_dropout / smx_backward_dropout with x, y, g, grad_x in the element
 * type `io` -- SMX_IO_F32 (exactly the f32 entries), SMX_IO_BF16 or SMX_IO_F16.  Everything else keeps its f32 type:
 * the filter, bias and their gradients, the saved spectrum xk, the workspace (same size).  Arithmetic is f32: the
 * 2-byte input is widened on load (exact), y / grad_x are rounded once at the store, to nearest even (a NaN stays a
 * NaN, fp16 overflow goes to +-inf) -- every output equals the f32 entry's output on the widened input, rounded to
 * `io`, bit for bit; xk and the parameter gradients equal the f32 entry's, bit for bit.
 * Native 2-byte I/O exists on the single-launch and residue-split plans with k <= 512 of the layer shapes
 * (smx_io_supported == 1).  Any other plan returns SMX_ERR_UNSUPPORTED: the caller widens the input itself and
 * calls the f32 entry.  Pointers: x / y / g / grad_x 4-byte aligned for a 2-byte `io` (8 for SMX_IO_F32).
 * Replaces: reference fft_tensor/spectral_layers.py:88-116 (the layer forward) and its autograd backward, in
 * bf16 / fp16 -- which the reference's torch.fft refuses (bf16) or runs in complex32 for powers of two only (fp16). */
#define SMX_IO_F32 0
#define SMX_IO_BF16 1
#define SMX_IO_F16 2
int smx_io_supported(int B, int N, int D, int F, int io);
int smx_forward_io(const void* x, const float* w_re, const float* w_im, const float* bias, void* y,
                   float* xk_save, void* workspace, size_t workspace_bytes, int B, int N, int D, int F,
                   int conj_w, float dropout_p, const void* rng_state, float* filter_pack, void* stream, int io);
int smx_backward_io(const void* g, const float* xk, const float* w_re, const float* w_im, void* grad_x,
                    float* gw_re, float* gw_im, float* gbias, void* workspace, size_t workspace_bytes, int B,
                    int N, int D, int F, int phases, float dropout_p, const void* rng_state,
                    const float* filter_pack, void* stream, int io);
int smx_block_forward_dropout(const float* x, const float* ln_w, const float* ln_b, float eps,
                              const float* w_re, const float* w_im, const float* bias, float* y,
                              float* xk_save, float* ln_stats, void* workspace,
                              size_t workspace_bytes, int B, int N, int D, int F, float dropout_p,
                              const void* rng_state, float* filter_pack, void* stream);
int smx_block_backward_dropout(const float* g, const float* x, const float* ln_stats,
                               const float* ln_w, const float* xk, const float* w_re,
                               const float* w_im, float* grad_x, float* g_ln_w, float* g_ln_b,
                               float* gw_re, float* gw_im, float* gbias, void* workspace,
                               size_t workspace_bytes, int B, int N, int D, int F, int phases,
                               float dropout_p, const void* rng_state, const float* filter_pack,
                               void* stream);
/* 2-byte activations of the block line: smx_block_forward_io / smx_block_backward_io are smx_block_forward_dropout /
 * smx_block_backward_dropout with x, y, g, grad_x in the element type `io` (SMX_IO_F32: exactly the f32 entries, grad_h
 * ignored).  The contract of smx_forward_io: arithmetic in f32, the 2-byte input widened exactly, y and grad_x rounded
 * once at the store to nearest even (a NaN stays a NaN, fp16 overflow goes to +-inf) -- y and grad_x equal the f32
 * entry's on the widened input, rounded to `io`, bit for bit; ln_stats, xk_save and all five parameter gradients equal
 * the f32 entry's, bit for bit.  Everything but the four activations keeps its f32 type; the workspace is the same.
 * grad_h: a (B, N, D) f32 scratch of the caller, 16-byte aligned, required for a 2-byte `io`: the gradient of the
 * LayerNorm's output stays f32 between the transform and the LayerNorm backward (a 2-byte grad_h would round it a
 * second time), so the backward is not in place.  Phase-split calls hand the same grad_h to every phase; the LayerNorm
 * backward belongs to SMX_PHASE_INVERSE as in smx_block_backward.
 * Native 2-byte block rows exist on the decimated single-launch plan (smx_plan: nsplit == 1, groups == 1, k <= 512, not
 * four-step / eight-band) with D % 4 == 0: smx_block_io_supported == 1 (for SMX_IO_F32 it is smx_block_supported(D)).
 * Any other shape returns SMX_ERR_UNSUPPORTED with nothing written: the caller widens the input and calls the f32 entry.
 * Pointers: x / y / g / grad_x 8-byte aligned for a 2-byte `io`.
 * Replaces: reference fft_tensor/spectral_layers.py:185 (x + spectral_mix(norm1(x)), with :154-158 and :162) and its
 * autograd backward in bf16 / fp16 -- there a torch LayerNorm, the layer and a torch add, each rounding the activation. */
int smx_block_io_supported(int B, int N, int D, int F, int io);
int smx_block_forward_io(const void* x, const float* ln_w, const float* ln_b, float eps, const float* w_re,
                         const float* w_im, const float* bias, void* y, float* xk_save, float* ln_stats,
                         void* workspace, size_t workspace_bytes, int B, int N, int D, int F, float dropout_p,
                         const void* rng_state, float* filter_pack, void* stream, int io);
int smx_block_backward_io(const void* g, const void* x, const float* ln_stats, const float* ln_w, const float* xk,
                          const float* w_re, const float* w_im, void* grad_x, float* g_ln_w, float* g_ln_b,
                          float* gw_re, float* gw_im, float* gbias, float* grad_h, void* workspace,
                          size_t workspace_bytes, int B, int N, int D, int F, int phases, float dropout_p,
                          const void* rng_state, const float* filter_pack, void* stream, int io);

/* The time path of fft_lm's BicameralBlock on the block's own (B, T, C) layout (round 4):
 *   y[b, t, c] = scale[b, c] * (bias[c] + w[c,0] x[b, t-2, c] + w[c,1] x[b, t-1, c] + w[c,2] x[b, t, c] * [t <= T-2])
 * replaces fft_lm/bicameral.py:214-223 (transpose, F.pad(x[:, :, :-1], (1, 0)), depthwise nn.Conv1d(kernel_size = 3,
 * padding = 1, groups = C), transpose back: the tap on x[t] is absent from the last row because the shifted sequence
 * dropped x[T-1]) and :226-227 (the time gate, as scale (B, C); NULL = 1), and their autograd backward.
 * w = conv1d.weight viewed as (C, 3); bias (C) or NULL.  Backward: grad_x (B, T, C) or NULL; grad_w (C, 3), grad_bias
 * (C), grad_scale (B, C): any may be NULL.  Fixed-order two-stage sums (bitwise reproducible); workspace from
 * smx_dwconv3_workspace_bytes, 256-byte aligned.  Pointers of (B, T, C) tensors 4-byte aligned (16-byte aligned and
 * C % 4 == 0 selects the vector kernels). */
int smx_dwconv3_workspace_bytes(int B, int T, int C, size_t* out);
int smx_dwconv3_forward(const float* x, const float* w, const float* bias, const float* scale, float* y, int B, int T,
                        int C, void* stream);
int smx_dwconv3_backward(const float* g, const float* x, const float* w, const float* bias, const float* scale,
                         float* grad_x, float* grad_w, float* grad_bias, float* grad_scale, void* workspace,
                         size_t workspace_bytes, int B, int T, int C, void* stream);

/* SpectralLayerNorm of fft_lm's FrequencyNativeBlock (round 4), replaces fft_lm/frequency_native.py:203-239 and its
 * autograd backward: per (batch row, bin) the magnitudes of the C channels are normalised (mean, biased variance, eps),
 * scaled by gamma[f, c], shifted by beta[f, c], and put back on the phases of z.
 *   z, out, g, grad_z: (B, F, C) complex64 (interleaved), 8-byte aligned; gamma, beta, grad_gamma, grad_beta: (F, C)
 *   float32 (rows of the module's (n_freqs, C) parameters: pass their base pointers, F <= n_freqs).
 * C <= 1024 (smx_spectral_ln_supported).  grad_z, grad_gamma, grad_beta may each be NULL.  Sums over the batch in a
 * fixed order (bitwise reproducible), no workspace. */
int smx_spectral_ln_supported(int C);
/* planar != 0: out (forward) / g (backward) are (2, B, F, C) float32 -- plane 0 the real parts, plane 1 the imaginary
 * parts -- instead of interleaved complex: the layout SpectralFFN's nn.Linear layers take ("the same weights on the real
 * and on the imaginary part", frequency_native.py:167-172), so no (de)interleaving copy stands between them. */
int smx_spectral_ln_forward(const float* z, const float* gamma, const float* beta, float eps, float* out, int planar,
                            int B, int F, int C, void* stream);
int smx_spectral_ln_backward(const float* g, const float* z, const float* gamma, const float* beta, float eps,
                             float* grad_z, float* grad_gamma, float* grad_beta, int planar, int B, int F, int C,
                             void* stream);
/* The planar side of SpectralFFN (frequency_native.py:167-189, :355-356), h / out / g (2, B, F, C) float32 planes:
 *   smx_planar_cmul_*: out = h (f_re + i f_im)[f, c] -- PhaseShift (:62-77) between the two Linear layers -- and its
 *     backward: grad_h = g conj(f), grad_f_re / grad_f_im (F, C) summed over the batch in a fixed order (any may be NULL);
 *   smx_planar_add: y = a + (p0 + i p1), y and a (n,) complex64 (a may be NULL): the residual around the feed-forward with
 *     the planar result folded in;  smx_planar_split: the two planes of a complex tensor (the backward of that fold). */
int smx_planar_cmul_forward(const float* h, const float* f_re, const float* f_im, float* out, int B, int F, int C,
                            void* stream);
int smx_planar_cmul_backward(const float* g, const float* h, const float* f_re, const float* f_im, float* grad_h,
                             float* grad_f_re, float* grad_f_im, int B, int F, int C, void* stream);
int smx_planar_add(const float* a, const float* planar, float* y, long long n, void* stream);
int smx_planar_split(const float* g, float* planar, long long n, void* stream);

/* The gate chain between the two transforms of fft_lm's twin blocks, one launch each way.  Replaces reference
 * fft_lm/frequency_native.py:95 (FrequencyConvFunc.forward: x k gain), :338 (times the frequency gate and the context
 * gate), :351 (times the cutoff mask) and their backward (:108-117 hand-written, the rest autograd); fft_lm/bicameral.py
 * :179-186 is the same product without u and m.
 *   forward:  y[b,f,c] = ((((x[b,f,c] a[f]) u[c]) p[f]) q[b,c]) m[f], multiplied in this (the reference's) order;
 *             x, y (B, F, C) complex64, a (F) complex64, u (C), p (F), q (B, C), m (F) float32; u, p, q, m may be NULL (= 1).
 *   backward: grad_x = g conj(a) u p q m (may be NULL) and three reductions the caller finishes with a few tiny products:
 *             s1 (F) complex64 = sum_{b,c} g conj(x) u q    -> grad_a = p m s1 (:111), grad_p = m Re(conj(a) s1)
 *             rc (B, C) = sum_f p m Re(conj(a) g conj(x))   -> grad_q = u rc; grad_u = sum_b q rc where autograd is meant
 *             rp (B, C) = sum_f p m Re(a g x)               -> the reference's own grad_gain = sum_b q rp (:115, un-conjugated)
 *             (s1, rc, rp may be NULL).  Sums in a fixed order: bitwise reproducible.
 * C must be even; x, y, g, grad_x 16-byte aligned; workspace as smx_spectral_gate_workspace_bytes says, 256-byte aligned. */
int smx_spectral_gate_workspace_bytes(int B, int F, int C, size_t* out);
int smx_spectral_gate_forward(const float* x, const float* a, const float* u, const float* p, const float* q,
                              const float* m, float* y, int B, int F, int C, void* stream);
int smx_spectral_gate_backward(const float* g, const float* x, const float* a, const float* u, const float* p,
                               const float* q, const float* m, float* grad_x, float* s1, float* rc, float* rp,
                               void* workspace, size_t workspace_bytes, int B, int F, int C, void* stream);

/* BicameralBlock's fusion line (reference fft_lm/bicameral.py:237-268: weighted paths + 0.1 x cross-talk + residual):
 *   forward:  out = r + w[0] a + w[1] b + c3 c   (n float32 each; w two floats in device memory; c may be NULL)
 *   backward: grad_a = w[0] g, grad_b = w[1] g, grad_c = c3 g (each may be NULL), grad_w[0] = sum g a, grad_w[1] = sum g b
 *             (fixed-order sums; may be NULL); grad_r is g itself.
 * n % 4 == 0, tensors 16-byte aligned; workspace as smx_mix_workspace_bytes says, 256-byte aligned. */
int smx_mix_workspace_bytes(size_t* out);
int smx_mix_forward(const float* r, const float* a, const float* b, const float* c, const float* w, float c3, float* out,
                    long long n, void* stream);
int smx_mix_backward(const float* g, const float* a, const float* b, const float* w, float c3, float* grad_a, float* grad_b,
                     float* grad_c, float* grad_w, void* workspace, size_t workspace_bytes, long long n, void* stream);

/* Row lines of EnhancedSpectralBlock (fft_tensor/spectral_enhancements.py:278-333), one launch each way:
 *   smx_rope_norm_*      line 1, :321 with RotaryFrequencyEmbedding :47-71 and nn.LayerNorm norm1 / norm2 (:305-306):
 *                          h1 = LN(x; ln1),  r = pairwise rotation of h1 by rotation[t] (complex64, (rot_rows, D/2)),
 *                          x1 = x + M1 r,  h2 = LN(x1; ln2);  stats (2, B, T, 2) = (mean, rstd) of both norms.
 *                        norm == 0: the standalone RotaryFrequencyEmbedding, x1 = rotation(x) (ln*, h2, stats unused).
 *                        Backward given g1 = dL/dx1 and gh2 = dL/dh2: G = g1 + LN2'(gh2), grad_x = G + LN1'(rot^T(M1 G)),
 *                        x1 recomputed from x in registers.  T > rot_rows -> SMX_ERR_INVALID.
 *   smx_residual_norm_*  the residual of line 2 and norm3 (:324, :327): x2 = x1 + M2 p,  h3 = LN(x2; ln3);
 *                        backward G = g2 + LN3'(gh3) -> grad_x1 = G, grad_p = M2 G (grad_p may be NULL without dropout:
 *                        it is then grad_x1).
 *   smx_gate_blend_*     line 3 after GatedSpectralUnit's two Linears (:105-114, :327): a (B, T, 2D) = gate_proj[0](h3),
 *                        v = value_proj(h3), ln (2D) = gate_proj[1]:  [z | vt] = LN(a),  gate = sigmoid(z),
 *                        x3 = x2 + M3 (gate v + (1 - gate) vt)  (x2 == NULL: the standalone unit, x3 = the blend);
 *                        backward: grad_v, grad_a (grad_x2 is g3 itself); stats (B, T, 2).
 * M = the library's dropout mask scaled by 1/(1 - p) (as the _dropout twins above: same words forward and backward,
 * element t D + d of batch row b).  ln_* may be NULL (no affine); gradient outputs g_ln_* may be NULL.  Even D <= 1024
 * (smx_enh_supported); every tensor 16-byte aligned; backward workspace from smx_enh_workspace_bytes, 256-byte aligned.
 * LayerNorm parameter gradients are summed in a fixed order: bitwise reproducible. */
int smx_enh_supported(int D);
int smx_enh_workspace_bytes(int B, int T, int D, size_t* out);
int smx_rope_norm_forward(const float* x, const float* rotation, int rot_rows, const float* ln1_w, const float* ln1_b,
                          const float* ln2_w, const float* ln2_b, float eps1, float eps2, float* x1, float* h2,
                          float* stats, int B, int T, int D, int norm, float dropout_p, const void* rng_state,
                          void* stream);
int smx_rope_norm_backward(const float* g1, const float* gh2, const float* x, const float* rotation, int rot_rows,
                           const float* ln1_w, const float* ln1_b, const float* ln2_w, const float* stats, float* grad_x,
                           float* g_ln1_w, float* g_ln1_b, float* g_ln2_w, float* g_ln2_b, void* workspace,
                           size_t workspace_bytes, int B, int T, int D, int norm, float dropout_p,
                           const void* rng_state, void* stream);
int smx_residual_norm_forward(const float* x1, const float* p, const float* ln_w, const float* ln_b, float eps,
                              float* x2, float* h3, float* stats, int B, int T, int D, float dropout_p,
                              const void* rng_state, void* stream);
int smx_residual_norm_backward(const float* g2, const float* gh3, const float* x2, const float* ln_w, const float* stats,
                               float* grad_x1, float* grad_p, float* g_ln_w, float* g_ln_b, void* workspace,
                               size_t workspace_bytes, int B, int T, int D, float dropout_p, const void* rng_state,
                               void* stream);
int smx_gate_blend_forward(const float* a, const float* v, const float* x2, const float* ln_w, const float* ln_b,
                           float eps, float* x3, float* stats, int B, int T, int D, float dropout_p,
                           const void* rng_state, void* stream);
int smx_gate_blend_backward(const float* g3, const float* a, const float* v, const float* ln_w, const float* ln_b,
                            const float* stats, float* grad_a, float* grad_v, float* g_ln_w, float* g_ln_b,
                            void* workspace, size_t workspace_bytes, int B, int T, int D, float dropout_p,
                            const void* rng_state, void* stream);

/* SpectralEMA, the frequency-domain state-space memory of fft_lm's chunk head, as one scan launch.
 *   smx_ema_scan_*    replace the per-step op sequence fft_lm/spectral_ssm.py:71-105 (update) and the Python loop over
 *                     the S chunks fft_lm/spectral_ssm.py:107-125 (scan): with rho = sigmoid(rho_logit[f]),
 *                     theta = pi tanh(theta_raw[f]), u(X) = X / |X| (u = 1 at X == 0),
 *                       SMX_EMA_ALIGNED:  H' = rho e^{i theta} |H| u(X) + (1 - rho) X
 *                       SMX_EMA_POLAR:    H' = (rho |H| + (1 - rho) |X|) u(X)        (theta_raw unused, may be NULL)
 *                     over t = 0 .. S-1 from H = init (B, F) (NULL: zeros); out (B, F) = the final state.  chunks (B, S, F),
 *                     init, out, g, grad_chunks, grad_init: interleaved complex64, 8-byte aligned; rho_logit, theta_raw,
 *                     their gradients: (F) float32 in DEVICE memory (read by the kernel: a captured graph sees updates).
 *   smx_ema_tokens_*  the same scan behind fft_lm/chunk_head.py:56-65: chunk t of row b is the L-point real DFT
 *                     (F = L / 2 + 1 bins, a direct sum) of tokens[b, t L : (t + 1) L] / 127.5 - 1, formed on the fly
 *                     -- the (B, S, F) spectrum never exists in memory.  2 <= L <= 64, S = T / L (trailing tokens are
 *                     ignored); token_bytes 1 (uint8) or 8 (int64); row_stride = elements between batch rows (>= T).
 *                     The DC and Nyquist bins are exact integer sums, and a run of equal bytes gives exactly zero in
 *                     every other bin; a bin that is exactly zero takes u = 1.
 * Backward (g = gradient of the final state): each output may be NULL.  The launch reruns the forward chain into the
 * workspace (smx_ema_workspace_bytes, 256-byte aligned: the (B, S, F) pre-step states and the per-chain parameter
 * gradients) and walks it in reverse; a second small launch sums the parameter gradients over the batch in a fixed
 * order -- bitwise reproducible.  The forward saves nothing and needs no workspace.  Where a state is exactly zero the
 * aligned step hands conj(rho e^{i theta} u(X)) G to it, as the reference's autograd does (angle's gradient is 0
 * there); SMX_EMA_POLAR writes zeros to grad_theta_raw.
 * S == 0: out = init (or zeros), grad_init = g, zero parameter gradients.  S < 0, L outside 2..64, a mode other than the
 * two, NULL required pointers: SMX_ERR_INVALID, nothing enqueued.  Nothing is allocated, the host is never synchronised. */
#define SMX_EMA_ALIGNED 0
#define SMX_EMA_POLAR 1
int smx_ema_workspace_bytes(int B, int S, int F, size_t* out);
int smx_ema_scan_forward(const float* chunks, const float* init, const float* rho_logit, const float* theta_raw,
                         float* out, int mode, int B, int S, int F, void* stream);
int smx_ema_scan_backward(const float* g, const float* chunks, const float* init, const float* rho_logit,
                          const float* theta_raw, float* grad_chunks, float* grad_init, float* grad_rho_logit,
                          float* grad_theta_raw, void* workspace, size_t workspace_bytes, int mode, int B, int S, int F,
                          void* stream);
int smx_ema_tokens_forward(const void* tokens, int token_bytes, long long row_stride, const float* init,
                           const float* rho_logit, const float* theta_raw, float* out, int mode, int B, int T, int L,
                           void* stream);
int smx_ema_tokens_backward(const float* g, const void* tokens, int token_bytes, long long row_stride, const float* init,
                            const float* rho_logit, const float* theta_raw, float* grad_init, float* grad_rho_logit,
                            float* grad_theta_raw, void* workspace, size_t workspace_bytes, int mode, int B, int T, int L,
                            void* stream);

/* The word-structure heads of fft_lm's bicameral trainer (fft_lm/phase_clock.py, fft_lm/segmentation_head.py).
 *   smx_word_targets  both target functions of byte tokens (B, T) in ONE launch without a host synchronisation, replacing
 *                     the per-byte `.item()` walk of fft_lm/phase_clock.py:83-113 (generate_phase_targets) and the
 *                     per-position op loop of fft_lm/segmentation_head.py:77-97 (get_word_boundaries).  tokens as in
 *                     smx_ema_tokens_* (token_bytes 1 = uint8 or 8 = int64, row_stride elements between rows, >= T); an
 *                     int64 value outside 0..255 is an ordinary word byte.
 *                       phase (B, T, 2), or NULL: with P = {32..47} u {58..64}, a word is a maximal run of non-P bytes
 *                         inside the row; position q of a word of length n gets (cos, sin)(pi q / (n - 1)) (n = 1: (1, 0)),
 *                         formed by sincospif(q / (n - 1)): a word start is exactly (1, 0); a byte of P gets (0, 0).
 *                         10 and 13, 91..96 and 123..126 are word bytes here.
 *                       boundary (B, T), or NULL: 1 where byte t + 1 is in S = P u {91..96} u {123..126} u {10, 13} and at
 *                         t = T - 1, else 0.
 *                     One workgroup per row: the delimiter bits of the row in LDS, a forward max-scan (last delimiter
 *                     before a 64-position word) and a backward min-scan (first one after it) over them, then the fill.
 *                     1 <= T <= 65536, B T < 2^31.  No atomics, no flags, no second launch.
 *   smx_head_*        the O-neuron row head, O = 1 or 2, replacing nn.Linear(d_model, 2) of fft_lm/phase_clock.py:53,65 and
 *                     nn.Linear(d_model, 1) of fft_lm/segmentation_head.py:43,55 over all R = B T rows of width C, float32:
 *                       y[r, o] = sum_e h[r, e] w[o, e] + b[o]           (b may be NULL)
 *                     one wavefront per row, the weight rows in registers.  Backward, one launch and the fixed-order
 *                     column sum of the LayerNorm gradients: grad_h[r, :] = sum_o g[r, o] w[o, :], grad_w[o, e] =
 *                     sum_r g[r, o] h[r, e], grad_b[o] = sum_r g[r, o] -- bitwise reproducible; each of grad_h, grad_w,
 *                     grad_b may be NULL (all NULL: nothing is enqueued).  h, grad_h: 16-byte aligned; C a width of the
 *                     LayerNorm row kernels (smx_head_supported(C, O) = smx_block_supported(C) and O in {1, 2}).
 *                     Workspace from smx_head_workspace_bytes, 256-byte aligned.
 * NULL required pointers, both target outputs NULL, token_bytes other than 1 or 8, misaligned int64 tokens,
 * row_stride < T, B, T or R <= 0, T > 65536: SMX_ERR_INVALID; O other than 1 or 2 or an unsupported C:
 * SMX_ERR_UNSUPPORTED; a missing, short or unaligned workspace: SMX_ERR_WORKSPACE.  Nothing is enqueued then, nothing is
 * ever allocated, the host is never synchronised. */
int smx_word_targets(const void* tokens, int token_bytes, long long row_stride, float* phase, float* boundary, int B,
                     int T, void* stream);
int smx_head_supported(int C, int O);
int smx_head_workspace_bytes(long long R, int C, int O, size_t* out);
int smx_head_forward(const float* h, const float* w, const float* b, float* y, long long R, int C, int O, void* stream);
int smx_head_backward(const float* g, const float* h, const float* w, float* grad_h, float* grad_w, float* grad_b,
                      void* workspace, size_t workspace_bytes, long long R, int C, int O, void* stream);

/* Softmax cross-entropy over the rows of a logits matrix: the two nn.functional.cross_entropy calls of compute_dual_loss,
 * fft_lm/dual_head.py:176-188 (256-way char loss; 50257-way token loss with ignore_index = 0), each logit read once per
 * direction and nothing of size R x V written in the forward.
 *   logits (R, V) float32, rows row_stride >= V elements apart; targets (R) int64; reduction SMX_XENT_MEAN / _SUM / _NONE.
 *   forward, for every row r with t_r != ignore_index:
 *       lse[r]  = log sum_j exp(x[r, j]), held as the pair (m, d) = (max_j x[r, j], log sum_j exp(x[r, j] - m))
 *       l[r]    = lse[r] - x[r, t_r] = d - (x[r, t_r] - m)
 *     lse (R, 2) floats is kept for the backward: m + d is the log-sum-exp, and the two stay apart because their sum
 *     rounded to one float loses d beside a large |m| (logits of 1e30: exp(x - lse) would be 1 where it is 1 / n);
 *     count[0] = number of rows that are not ignored, as a float (exact below 2^24
 *     rows); loss = sum_r l[r] / count (MEAN), sum_r l[r] (SUM): one float, or l itself (NONE): R floats.  An ignored
 *     row is not read: its l[r] and its lse pair are 0.
 *   backward: grad[r, j] = (exp((x[r, j] - m) - d) - [j == t_r]) s_r, grad (R, V) dense, with s_r = g[0] / count[0]
 *     (MEAN), g[0] (SUM), g[r] (NONE): g and count are read from device memory by the kernel, no scalar crosses to the
 *     host.  An ignored row is not read and its gradient row is written as zeros (never multiplied: with every row ignored
 *     the mean is 0 / 0 = NaN and the gradient is all zeros).
 *   Edge semantics: -inf entries are ordinary (the loss is finite when any entry is finite); a row with +inf, or with
 *     -inf only, has a NaN loss.  DIFFERENCE FROM TORCH: a target outside [0, V) that is not ignore_index -- a device-side
 *     assert there -- makes that row's loss and its whole gradient row NaN here; the row is counted, and no address is
 *     ever formed from the target.
 *   Kernels: V a LayerNorm row width (V <= 4096 with V % 4 == 0, V <= 1024 otherwise): one wavefront per row, the row in
 *     registers; its 16-byte chunks need logits, grad and row_stride * 4 to be multiples of 16 bytes -- otherwise the
 *     call takes the one-element-per-lane instance (V <= 1024) or the streaming kernels, never a misaligned vector access.
 *     Every other V up to 2^31 - 1: one workgroup of 256 threads per row, a running (max, sum) per thread merged in a
 *     fixed order, scalar head up to 16-byte alignment, 16-byte body, scalar tail; row offsets are 64-bit.
 *   The sum over rows: one (sum, count) partial per workgroup in the workspace, added in index order by a second,
 *     one-workgroup launch: no atomics, no flags, bitwise reproducible.  smx_xent_supported(V) = V >= 1.
 * NULL required pointers, R <= 0, V <= 0, row_stride < V, an unknown reduction, pointers that are not 4-byte (targets:
 * 8-byte) aligned: SMX_ERR_INVALID; a missing, short or unaligned workspace (smx_xent_workspace_bytes, 256-byte aligned;
 * forward only): SMX_ERR_WORKSPACE.  Nothing is enqueued then, nothing is ever allocated, the host is never synchronised. */
#define SMX_XENT_MEAN 0
#define SMX_XENT_SUM 1
#define SMX_XENT_NONE 2
int smx_xent_supported(int V);
int smx_xent_workspace_bytes(long long R, int V, size_t* out);
int smx_xent_forward(const float* logits, long long row_stride, const long long* targets, long long ignore_index,
                     int reduction, float* loss, float* lse, float* count, void* workspace, size_t workspace_bytes,
                     long long R, int V, void* stream);
int smx_xent_backward(const float* g, const float* logits, long long row_stride, const long long* targets,
                      long long ignore_index, int reduction, const float* lse, const float* count, float* grad,
                      long long R, int V, void* stream);

/* Overlap-save chunk generation: one chunk step of a FixedSpectralBlock at inference as two row-kernel launches
 * around the block's gate_ctx GEMV (which stays the caller's), replacing the per-chunk op sequence of
 * scripts/generate_chunked_overlap_save.py:101-172 (LayerNorm of the chunk, a torch.cat of the whole (Bt, T, C) window,
 * a full sum over it, an rfft and an irfft of n_fft points x C channels of which `chunk` rows are kept, and about a
 * dozen pointwise launches).  At inference the filter spectrum k_freq sigmoid(gate_freq) (x cutoff mask) is a
 * constant; h_eff = its n_fft-point inverse transform is a real constant too, and the kept rows of the reference's
 * circular convolution are a (chunk x (K - 1 + chunk)) Toeplitz slice of h_eff -- negative lags (the circular wrap of
 * the gated, non-compact h_eff) included -- applied to the last K - 1 + chunk rows of the window.
 * State per layer, float32 (pos: int32) in DEVICE memory, owned by the caller:
 *     ring (Bt, T, C)   the window of LayerNorm outputs, a ring buffer that is never copied
 *     sum  (Bt, 2, C)   the window sum as a compensated pair (hi, lo)
 *     pos  (Bt)         slot of the oldest row = the next write slot (read by the kernels: a captured graph replays
 *                       correctly as the ring turns)
 *   smx_stream_push   (:101-115) for n < chunk: slot = (pos[b] + n) % T, the evicted row is read, LayerNorm(h[b, n];
 *                     ln_w, ln_b, eps) is written there and new - evicted accumulated; the sums of the block's
 *                     wavefronts are added in wavefront order (bitwise reproducible) and folded into (hi, lo) by a
 *                     two-sum; then pooled[b] = (hi + lo) / T and pos[b] = (pos[b] + chunk) % T.  One workgroup per
 *                     batch row, the only reader and writer of that row's pos: no atomics.  h (Bt, chunk, C),
 *                     pooled (Bt, C); ln_w / ln_b may be NULL.
 *   smx_stream_conv   (:118-172 up to the FFN's linears) with pos already advanced, L = K - 1 + chunk,
 *                     seg[j] = ring[b, (pos[b] - L + j) mod T]:
 *                       y[n] = sum_{j < L} taps[n + L - 1 - j] seg[j]
 *                       h_out[b, n] = h[b, n] + scale[b] * y[n]          scale (Bt, C) = gain * g_ctx
 *                       ff_in[b, n] = LayerNorm(h_out[b, n]; ln_w, ln_b, eps)     (ff_in == NULL: skipped)
 *                     taps: K + 2 chunk - 2 floats, taps[i] = h_eff[(i - (chunk - 1)) mod n_fft] -- the library never
 *                     sees n_fft.  h_out may be h.
 *   smx_stream_supported(T, K, C, chunk): 1 when C is a width of the LayerNorm row kernels (smx_block_supported),
 *                     1 <= chunk <= 64, 1 <= K <= 4096 and K - 1 + chunk <= T.
 * NULL required pointers, tensors that are not 16-byte aligned (pos and taps, which no vector load touches: 4-byte),
 * Bt < 1 or an unsupported shape:
 * SMX_ERR_INVALID, nothing enqueued.  Nothing is allocated, the host is never synchronised. */
int smx_stream_supported(int T, int K, int C, int chunk);
int smx_stream_push(const float* h, const float* ln_w, const float* ln_b, float eps, float* ring, float* sum, int* pos,
                    float* pooled, int Bt, int T, int C, int chunk, void* stream);
int smx_stream_conv(const float* h, const float* ring, const int* pos, const float* taps, const float* scale,
                    const float* ln_w, const float* ln_b, float eps, float* h_out, float* ff_in, int Bt, int T, int K,
                    int C, int chunk, void* stream);

/* The byte sampler of generation: one launch for the penalties, bans, temperature, nucleus, top-k and the draw that the
 * reference spreads over Python loops and about a dozen small ops with several host synchronisations per byte --
 * fft_lm/train_fixed_full.py:651-701 (generate), scripts/stream_generate_fast.py:146-170 (sample_next),
 * scripts/generate_chunked_overlap_save.py:39-48 and :283-292 and its siblings.  They are one function of a row of 256
 * logits; per row r of R, in this order (the reference's results depend on it):
 *    1  l = logits[r, :]                                     float32, rows row_stride >= 256 elements apart
 *    2  for every byte b present in recent:  l[b] /= repetition_penalty      (a plain division, for negative logits too)
 *    3  if presence_penalty or frequency_penalty is not 0:  l[b] -= presence_penalty + frequency_penalty * count[b]
 *    4  ascii_only: everything but 10 and 32..126 becomes -inf;  ban_cr: 13 becomes -inf
 *    5  max_run_length > 0, n_recent >= max_run_length and the last max_run_length ids of recent all equal: that byte
 *       becomes -inf
 *    6  l /= temperature
 *    7  top_p < 1: in descending order of l (equal logits by index), the longest prefix whose running softmax sum stays
 *       <= top_p is kept, at least one entry; the rest becomes -inf.  top_p >= 1: no such step.
 *    8  top_k > 0: with v the min(top_k, 256)-th largest remaining value, every l < v becomes -inf
 *    9  p = softmax(l)
 *   10  ids[r] = the first j, in index order, with sum_{i <= j} p_i > u[r]
 *   recent: n_recent ids shared by all rows of the call, uint8 or int64 (token_bytes 1 or 8, as smx_word_targets; an
 *   int64 id outside 0..255 counts for no byte), 0 <= n_recent <= 65536; u (R) float32 uniforms in [0, 1); ids (R)
 *   int64; probs (R, 256) float32 dense, or NULL: the distribution of step 9.
 *   Guarantees: p[ids[r]] > 0 always -- where rounding leaves u above the last running sum, the last byte with p > 0 is
 *   taken; a NaN logit gives an unspecified id in [0, 255] and no fault.  One workgroup of 256 threads per row, every sum
 *   a block scan in a fixed order: bitwise reproducible, and a row's result does not depend on the other rows.  No
 *   atomics on global memory, no flags.
 * smx_sample_supported(V) = (V == 256); any other V: SMX_ERR_UNSUPPORTED.  R <= 0, NULL logits / u / ids (recent with
 * n_recent > 0), row_stride < 256, token_bytes other than 1 or 8, n_recent outside [0, 65536], misaligned pointers,
 * temperature or repetition_penalty not positive and finite, a NaN top_p, non-finite penalties, negative top_k or
 * max_run_length: SMX_ERR_INVALID.  Nothing is enqueued then, nothing is ever allocated, the host is never synchronised. */
int smx_sample_supported(int V);
int smx_sample_bytes(const float* logits, long long row_stride, const void* recent, int token_bytes, int n_recent,
                     float temperature, float top_p, int top_k, float repetition_penalty, float presence_penalty,
                     float frequency_penalty, int ascii_only, int ban_cr, int max_run_length, const float* u,
                     long long* ids, float* probs, long long R, int V, void* stream);

/* The byte-spectral feature rows of fft_tensor's byte language model: what ByteSpectralEmbedding.forward
 * (fft_tensor/byte_spectral_model.py:44-102) builds with a Python loop over all T positions -- roll, a full FFT, abs,
 * angle, a multiply, sin, cos, cat and a pad per position, about ten launches each -- and ByteSpectralEncoder.forward
 * (fft_tensor/byte_spectral.py:53-108) once per sequence, both up to their projection, as ONE launch.
 *   tokens (B, T) as in smx_word_targets (token_bytes 1 = uint8 or 8 = int64, row_stride >= T elements between rows); ANY
 *   int64 value is converted as the reference's .float() does.  s[t] = id[t] / 127.5 - 1, S[f] = sum_t s[t]
 *   e^{-2 pi i f t / T}.  The spectrum of roll(s, -pos) is S[f] e^{i theta}, theta = 2 pi (f pos mod T) / T, so with
 *   u = S / |S| column j of out[b, p, :] (pos = p; P = 1: pos = 0) is
 *       0 <= j <  k     |S[b, j]| bands[j]
 *       k <= j < 2k     Im(u[b, j - k] e^{i theta})          = sin(angle(spectrum of the rolled row))
 *      2k <= j < 3k     Re(u[b, j - 2k] e^{i theta})         = cos(...)
 *      3k <= j < W      0
 *   cut at W columns.  A bin with S == 0 exactly has sin 0 and cos 1 at every position (torch's angle(0) = 0); nothing is
 *   ever NaN.  out (B, P, W) float32, P = T (row p is position p: the embedding, k = min(W / 2, T / 2)) or P = 1 (the
 *   encoder, W = 2 M, k = min(M, T / 2)); bands: at least k floats; mag (B, k), or NULL: |S|, what the backward needs.
 *   Accuracy: every twiddle, the rotation included, is entry (f t mod T) -- the exact integer -- of one T-entry table
 *   built by sincospi in double; the row enters as the integers 2 id - 255 (for f > 0 minus the row's mean rounded to an integer,
 *   which changes no bin, keeps the partial sums small and makes a constant row an exact zero); each bin is summed over slices with four interleaved
 *   accumulators and the slices joined pairwise.
 *   One launch, no host synchronisation, capturable; a workgroup recomputes its row's k bins from the bytes in LDS and
 *   writes a chunk of positions (16, more once B alone fills the chip; T > 512: at least T / 32) as 16-byte vectors when
 *   W % 4 == 0.
 *   smx_byte_supported(T, k, W) = 1 <= T <= 4096, 0 <= k <= min(T / 2, 2048), 1 <= W <= 4096 (no HIP call).
 *   smx_byte_grad_bands  grad_bands[f] = sum_b sum_p g[b, p, f] mag[b, f] for f < min(k, W), 0 for min(k, W) <= f <
 *   n_bands; g (B, P, W) dense.  Two plain launches: per (b, 64 rows) partials in the workspace
 *   (smx_byte_workspace_bytes, 256-byte aligned), then their sum in index order: no atomics, bitwise reproducible.
 * B, T, W, P <= 0 or k < 0, token_bytes other than 1 or 8, P other than 1 or T, k > T / 2, NULL required pointers,
 * row_stride < T, misaligned int64 tokens, out not 16-byte aligned, n_bands < max(1, min(k, W)): SMX_ERR_INVALID; a size
 * outside smx_byte_supported: SMX_ERR_UNSUPPORTED; a missing or short workspace: SMX_ERR_WORKSPACE.  Nothing is enqueued
 * then, nothing is ever allocated, the host is never synchronised. */
int smx_byte_supported(int T, int k, int W);
int smx_byte_features(const void* tokens, int token_bytes, long long row_stride, const float* bands, float* out,
                      float* mag, int B, int T, int k, int W, int P, void* stream);
int smx_byte_workspace_bytes(int B, int P, int W, int k, size_t* out);
int smx_byte_grad_bands(const float* g, const float* mag, float* grad_bands, int n_bands, void* workspace,
                        size_t workspace_bytes, int B, int P, int W, int k, void* stream);

/* Multi-pattern exact byte search: the `corpus_bytes.find(snip)` loop of the trainer's parroting_score
 * (fft_lm/train_fixed_full.py:185-205: one host scan of the whole corpus per absent snippet, up to 64 per epoch) as ONE
 * pass over the corpus that tests all snippets at every position.
 *   corpus: n bytes, ANY alignment.  snips: S snippets of L bytes each, contiguous (S, L).  first (S) int64:
 *   first[s] = the smallest p in [0, n - L] with corpus[p : p + L] == snips[s], -1 if there is none -- bytes.find.
 *   Identical snippets each get their answer.  n < L (n == 0 too, corpus may then be NULL): every answer is -1, still
 *   written on the stream.
 *   Two launches: persistent workgroups walk 16384-position tiles (aligned to 16-byte addresses; 16-byte loads for
 *   every vector wholly inside the corpus, byte loads at its two ends, nothing outside [corpus, corpus + n) and
 *   [snips, snips + S L) is read), test each position's 4-byte window against an LDS bitmap of the snippets' hashed first
 *   words and verify hits from LDS; each workgroup's minima go to its row of a table in the workspace, and a second
 *   launch takes the column minima (one workgroup per snippet).  No flag words, no atomics on memory, no workgroup waits for another:
 *   the result is a pure function of the inputs, bitwise reproducible.  max_workgroups: 0 = as many as stay resident,
 *   n > 0 caps the scan at n workgroups (tests force the tile walk with 1 or 2).
 *   smx_match_supported(S, L) = 1 <= S <= 256, 4 <= L <= 256, S L <= 32768 (no HIP call).
 * A set outside smx_match_supported: SMX_ERR_UNSUPPORTED; n < 0, NULL snips / first / (n > 0) corpus, first not 8-byte
 * aligned, max_workgroups < 0: SMX_ERR_INVALID; a missing, short or unaligned workspace (smx_match_workspace_bytes,
 * 256-byte aligned): SMX_ERR_WORKSPACE.  Nothing is enqueued then, nothing is ever allocated, the host is never
 * synchronised; the call can be captured in a graph. */
int smx_match_supported(int S, int L);
int smx_match_workspace_bytes(int S, int L, size_t* out);
int smx_match_first(const void* corpus, long long n, const void* snips, int S, int L, long long* first, void* workspace,
                    size_t workspace_bytes, int max_workgroups, void* stream);

/* The two native ops of the sparse spectral tensor (fft_tensor/tensor.py:136-144 _sparsify_pytorch: abs, topk, >=,
 * nonzero, masked gather; fft_tensor/tensor.py:194-203 _scatter_pytorch: fill + index_put; the extension that
 * fft_tensor/setup.py:20-49 declares for them was never written).  For n complex64 values z[i] = (re, im), 8-byte aligned at any 8-byte offset:
 *   key[i] = bits(fl(fl(re re) + fl(im im))) & 0x7fffffff   (fp32, round to nearest, no FMA), compared as unsigned;
 *   T = the k-th largest key (1 <= k <= n); kept = {i : key[i] >= T}: m >= k, ties at T are all kept; a NaN key ranks
 *   above inf.
 * smx_topk_select: an exact radix select over the 31 key bits in three passes over z (digits of 11, 10, 10 bits: LDS
 *   histograms per workgroup, rows in the workspace, a column-sum launch and a one-workgroup pick per pass), then the
 *   kept elements are counted per 4096-element tile (a fourth pass) and the counts scanned.  result (2 int64 on the
 *   device): result[0] = m, result[1] = T.
 * smx_topk_compact: one more pass writes the first min(m, capacity) kept elements in ascending index order (the order
 *   of torch.nonzero): coeffs[j] (complex64) and flat_idx[j] (int64).  It reads `result` and the tile offsets that the
 *   preceding smx_topk_select of the same z and n left in the same workspace (any max_workgroups: offsets are per tile).
 * smx_sparse_scatter: out (n complex64, 16-byte aligned) = zeros with out[flat_idx[j]] = coeffs[j], j < m, in ONE launch
 *   that writes `out` exactly once with 16-byte stores (tiles built in LDS; each workgroup finds its first entry by binary
 *   search) and reads nothing of size n.  flat_idx must be strictly ascending and in [0, n): the caller's promise.  If it
 *   is broken the contents of `out` are unspecified, but nothing outside `out` is written.  m = 0 (coeffs and flat_idx
 *   may then be NULL) is a plain fill.
 * No flag words, no atomics on memory, no workgroup waits for another: every result is a pure function of the inputs,
 * bitwise reproducible.  max_workgroups: 0 = as many as stay resident, n > 0 caps every tile walk at n workgroups
 * (tests force the walk with 1 or 2).  smx_topk_supported(n) = 1 <= n < 2^31 (no HIP call).
 * n outside smx_topk_supported: SMX_ERR_UNSUPPORTED; NULL pointers, k outside 1..n, m outside 0..n, capacity < 0,
 * max_workgroups < 0, z / result / coeffs / flat_idx not 8-byte or out not 16-byte aligned: SMX_ERR_INVALID; a missing,
 * short or unaligned workspace (smx_topk_workspace_bytes, 256-byte aligned): SMX_ERR_WORKSPACE.  Nothing is enqueued
 * then, nothing is ever allocated, the host is never synchronised; the calls can be captured in a graph. */
int smx_topk_supported(long long n);
int smx_topk_workspace_bytes(long long n, size_t* out);
int smx_topk_select(const void* z, long long n, long long k, long long* result, void* workspace, size_t workspace_bytes,
                    int max_workgroups, void* stream);
int smx_topk_compact(const void* z, long long n, const long long* result, void* coeffs, long long* flat_idx,
                     long long capacity, void* workspace, size_t workspace_bytes, int max_workgroups, void* stream);
int smx_sparse_scatter(const void* coeffs, const long long* flat_idx, long long m, void* out, long long n,
                       int max_workgroups, void* stream);

#ifdef __cplusplus
}
#endif

/* Entry points added after the table of this header's signatures was recorded live in headers of their own, included
 * here: a C caller sees one ABI, and the Python binding reads each header it names (_lib.EXT_HEADERS, and
 * _lib.MORE_HEADERS for the ones after smx_freq.h, whose table is recorded as it stood too). */
#include "smx_freq.h"
#include "smx_fconv.h"
#include "smx_quant.h"
#include "smx_rowfft.h"

#endif /* SMX_H_ */
