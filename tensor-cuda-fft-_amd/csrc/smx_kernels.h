// smx_kernels.h -- launch-side declarations shared by the kernel translation units and smx_api.
#pragma once
#include <hip/hip_runtime.h>
#include "smx_core.h"

namespace smx {

// ---- supported-value sets, stated once: the plans (smx_api.hip) ask has(), the launchers pick from the same list --------
// among<Vs...>{v}: a run-time value that selects a template argument from Vs (pick_key, smx_launch.h)
template <int... Vs>
struct among {
  int v;
  static constexpr bool has(int x) { return ((x == Vs) || ...); }
};
struct flag { bool v; };       // ... and one that selects a bool template argument
// four-step tile counts L = n_fft / 256 whose column transform one thread holds in registers (k_fs_f<L, .>): 2 and 4
// for the complex sequence FFT alone, the filter plans from FS_FILTER_MIN_L (below it their band kernels are faster)
using fs_one_level = among<2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28,
                           29, 30, 31, 32>;
constexpr int FS_FILTER_MIN_L = 5;
// ... of them, those whose mode-1 launch can sum the slab rows over batch groups (k_fs_f_grouped<L>, option fs_bgroups)
using fs_grouped_tiles = among<5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>;
// two-level columns (k_fs_big<L2, ., L1>): L = L1 L2 with L2 threads per column pair and a first-level length 9 ... 16,
// the smallest such L2 -- 36 ... 64 step 4, 72 ... 128 step 8, 144 ... 256 step 16
using fs_level2 = among<4, 8, 16>;
using fs_level1 = among<9, 10, 11, 12, 13, 14, 15, 16>;
constexpr bool fs_two_level(int L, int* L1, int* L2) {
  for (int l2 = 4; l2 <= 16; l2 *= 2)
    if (fs_level2::has(l2) && L % l2 == 0 && fs_level1::has(L / l2)) { *L1 = L / l2; *L2 = l2; return true; }
  return false;
}
constexpr bool fs_tiles_cfft(int L) { int l1 = 0, l2 = 0; return fs_one_level::has(L) || fs_two_level(L, &l1, &l2); }
constexpr bool fs_tiles_filter(int L) { return L >= FS_FILTER_MIN_L && fs_tiles_cfft(L); }
// rank-one filter (launch_fs_conv): columns in one thread's registers (k_fs_conv<L, .>; L = 32 was measured: 512 registers
// + 116 spills in backward, no faster than k_fs_f), above that L = 16 L2 on the two-level columns (k_fs_conv_big<L2, .>)
using conv_one_level = among<2, 4, 8, 16>;
using conv_level2 = among<2, 4, 8, 16>;
constexpr bool conv_two_level(int L) { return L % 16 == 0 && conv_level2::has(L / 16); }
constexpr bool conv_tiles(int L) { return conv_one_level::has(L) || conv_two_level(L); }
// k_conv1<LP, ...>: n_fft = 512 LP
using conv1_lp = among<1, 2, 4>;
constexpr bool conv1_length(int N) { return N % 512 == 0 && conv1_lp::has(N / 512); }

struct DecimArgs {
  const float* in;      // x (forward) or g (backward), (B,N,D) f32 -- or 2-byte rows behind the same pointer (io below)
  float* out;           // y or grad_x, (B,N,D) likewise; may be null (spectrum only)
  const cf* tw;         // w_N^n, n < N
  const cf* bt;         // w_N^{16 s' r}, [L][32]
  const cf* tq;         // w_N^{q e}, [N/16][16] (N % 256 == 0): the inter-pass twiddles c^q of row-group t and residue
                        // r at row e = t L + r, read by the streaming loops instead of raising c to its powers
  Geom g;
  FilterArgs fa;
  const cf* v16;        // sixteen-row decimation (g.P != 0): V[s'' + 16][t'] = w_P^{s'' t'}, 32 x 16
  const cf* b16;        // ... and beta[tau][s'' + 16] = w_P^{16 s'' tau}, T x 32
  int placement;        // workgroup placement: 0 b-major, 1 + rotated residues, 2 XCD-aware (default)
  int accumulate;       // four-band kernels only: out += instead of out = (band groups after the first)
  int round;            // workgroups per launch of the streaming kernels (0 = all in one launch)
  int st_plain;         // 0, 1, 2 or 4: rows of every tile (of a thread's 16) stored write-back, the others streaming
  // which ones (store_rows, smx_launch.h): row u of tile r in wave w is write-back iff bit u of
  // rot16(st_mask, (r >> st_rsh) + (w >> st_wsh)) is set; store_layout() below fills the three from the option
  unsigned st_mask;
  int st_rsh, st_wsh;
  int bid0;            // first workgroup index of this launch (set by the launchers)
  // split path only
  int nsplit, lc;       // residues are cut into nsplit chunks of lc
  int sum_in_f;         // 1: k_split_f sums the chunk partials itself (no k_split_sum launch)
  cf* ws_z;             // [B*ndt][nsplit][16 NB][256] partial packed spectra
  cf* ws_zs;            // [B*ndt][16 NB][256] partial spectra summed over the chunks
  cf* ws_s;             // [B*ndt][16 NB][256] filtered packed spectra
  const float* out_scale;  // k_fs_b: (B, D) factors applied to the two channels at the store, or null
  ConvArgs ca;          // rank-one filter on the four-step path (launch_fs_conv)
  const cf* conv_src;   // launch_fs_conv: where the columns are read (ws_f itself, or the saved spectra of x)
  int fs_bgroups;       // four-step backward: batch groups whose slab rows are summed inside k_fs_f (0 = per row)
  cf* ws_f;             // four-step path: [B*ndt][L][16][256] per-residue tile spectra (in place: filtered)
  // dropout (training): mask regenerated from (rng[0], rng[1]) = (seed, call counter) in device memory;
  // forward launches apply it to what they store, backward launches to the g they load
  unsigned drop_thr;    // round(p * 65536); 0 = none
  float drop_scale;     // 65536 / (65536 - drop_thr)
  const unsigned long long* rng;
  // fused block (launch_fused_block only): in = x, LayerNorm folded into the load, + x at the store
  const cf* ln_stats;   // (B,N) (mean, rstd)
  const float* ln_w;    // (D) or null (= 1)
  const float* ln_b;    // (D) or null (= 0)
};

// Placement of the a.st_plain write-back rows of a tile (option "st_layout").  rot16(m, s): bit u
// of the result = bit (u + s) mod 16 of m, so with the base mask of period 16 / count (0x1111, 0x0101, 0x0001) row u is
// write-back iff (u + s) mod (16 / count) == 0.  s per layout (r = tile residue, w = wave of the workgroup = t >> 2):
//   -1  the thread's FIRST rows u < count, no rotation: one contiguous count/16 of every batch row (1 MiB of 4 at C2)
//    0  s = 0: rows u = 0 (mod 16 / count), count blocks of 1/16 of the batch row (256 KiB)
//    1  s = r: pieces of one row (D elements, 1 KiB)        2  s = r >> 2: four rows (4 KiB)
//    3  s = w: the 4 L rows of one wave (64 KiB), another u in every 16 L-row window
//    4  s = w + r: single rows again, also rotated by wave
// A shift of 30 switches a term off (r and w are small non-negative numbers).
static inline void store_layout(DecimArgs& a, int layout) {
  const int c = a.st_plain;
  a.st_rsh = a.st_wsh = 30;
  if (layout < 0 || layout > 4) { a.st_mask = (1u << c) - 1u; return; }
  a.st_mask = c == 4 ? 0x1111u : c == 2 ? 0x0101u : c == 1 ? 0x0001u : 0u;
  if (layout == 1 || layout == 4) a.st_rsh = 0;
  if (layout == 2) a.st_rsh = 2;
  if (layout == 3 || layout == 4) a.st_wsh = 0;
}

// sixteen-row decimation (N % 16 == 0, N % 256 != 0, k <= 128 nb): one launch per direction, modes as launch_fused
hipError_t launch_fused16(const DecimArgs& a, int nb, int mode, hipStream_t s);
// ... its residue-split form for few (batch row, d-tile) pairs: (A) partial spectra per chunk of tiles, then
// launch_split_f (shared with the 256-point plan), then (B) the inverse per chunk; (B) with nsplit == 1 is also the
// inverse half of a phase-split backward (from the spectrum launch_fused16 with out == NULL parked in ws_s)
hipError_t launch_split16_a(const DecimArgs& a, int nb, bool drop_in, hipStream_t s);
hipError_t launch_split16_b(const DecimArgs& a, int nb, bool drop_out, hipStream_t s);
// fused single-launch path (nsplit == 1)
// io (here and in launch_split_a / launch_split_b): element type of the rows a.in / a.out point at (SMX_IO_*: 0 f32,
// 1 bf16, 2 fp16 -- 2-byte rows, everything else f32).  io != 0 exists for modes 0 and 1 without zero-padded rows
// or band groups (accumulate); anything else: hipErrorInvalidValue
// oio: element type of a.out where it differs from a.in's (-1 = io).  Only (io 2-byte, oio f32, mode 1) exists: the
// block backward, whose grad_h stays f32 for the LayerNorm backward behind it
hipError_t launch_fused(const DecimArgs& a, int nb, int mode, hipStream_t s, int io = 0, int oio = -1);
// synthesis from a given one-sided spectrum (fa.xk_in, fa.sp_scale, fa.sp_herm): fused inverse, or the packed
// spectrum parked for launch_split_b when out == NULL
hipError_t launch_synth(const DecimArgs& a, int nb, hipStream_t s);
hipError_t launch_synth8(const DecimArgs& a, hipStream_t s);       // N = 2048, every bin: eight bands, one launch
// full spectrum at N = 2048 (eight bands, L == 8): one launch per direction, no dropout / residue split
hipError_t launch_full8(const DecimArgs& a, int mode, hipStream_t s);
// four-step path (more than 512 bins at the tile counts of fs_tiles_filter above): tile spectra -> workspace / column
// filter / inverse
hipError_t launch_fs_a(const DecimArgs& a, hipStream_t s);
hipError_t launch_fs_f(const DecimArgs& a, int mode, hipStream_t s);     // mode 4: columns from fa.xk_in (synthesis)
hipError_t launch_fs_b(const DecimArgs& a, hipStream_t s);
int conv_column_blocks(int L);      // the same for launch_fs_conv (ConvArgs::r_part)
int fs_column_blocks(int L);        // grid.y of the column launch = rows of FilterArgs::gsc_part per workgroup
hipError_t launch_fs_big_general(const DecimArgs& a, int mode, int l1, int l2, hipStream_t s);   // L1 = 9 ... 15
// rank-one filter (causal convolution of fft_lm) on the four-step path: column launch, dir 0 forward / 1 backward
// (backward also reduces P -> dL/dH (gh_re, gh_im: N/2 + 1 each) and (R1, R2) -> grad_scale (B, D))
hipError_t launch_fs_conv(const DecimArgs& a, int dir, float* gh_re, float* gh_im, float* grad_scale,
                          hipStream_t s);
hipError_t launch_conv_reduce(const DecimArgs& a, float* gh_re, float* gh_im, float* grad_scale, int ny,
                              float rscale, hipStream_t s, int nwg = 0, int nj = 16);
// the same filter in ONE launch per direction (smx_conv1.hip): n_fft = 512, 1024, 2048 (rows above n_fft / 2 folded).
// dir 0: a.ws_f = where the packed spectrum of x is kept for backward (or null); dir 1: a.ca.xs = that spectrum,
// partial sums as launch_fs_conv with one row of (R1, R2) per workgroup
constexpr bool conv1_supported(int N, int R) { return conv1_length(N) && R >= 1 && R <= N; }
// nj = channel pairs per workgroup: 16 (512 threads) or 8 (256 threads, two workgroups per CU)
int conv1_workgroups(int B, int D, int nj);
// io: element type of a.in / a.out (SMX_IO_*: 0 f32 rows, 1 bf16, 2 fp16 -- 2-byte rows, everything else f32)
hipError_t launch_conv1(const DecimArgs& a, int nj, int dir, float* gh_re, float* gh_im, float* grad_scale,
                        hipStream_t s, int io = 0);
// the filter's own response H = rfft(zero-pad(kernel), N) * sigmoid(logits) * mask (f <= N/2) and its backward
hipError_t launch_conv_response(const float* kernel, const float* logits, const float* mask, const cf* tw, int N,
                                int K, float* h_re, float* h_im, hipStream_t s);
hipError_t launch_conv_response_bwd(const float* kernel, const float* logits, const float* mask, const cf* tw, int N,
                                    int K, int n_logits, const float* gh_re, const float* gh_im, float* grad_kernel,
                                    float* grad_logits, hipStream_t s);
// W[d, f] = c_f m[d] exp(i p[d]) (PhaseAwareSpectralMixing) and the gradients of m, p from grad_W (row pitch ld)
hipError_t launch_phase_filter(const float* m, const float* ph, int D, int k, int n_fft, float* w_re, float* w_im,
                               hipStream_t s);
hipError_t launch_phase_filter_bwd(const float* m, const float* ph, const float* gw_re, const float* gw_im, int D, int k,
                                   int n_fft, int ld, float* g_m, float* g_p, hipStream_t s);
// forward of y = x + mix(LayerNorm(x)) in one launch (nsplit == 1 only)
hipError_t launch_fused_block(const DecimArgs& a, int nb, hipStream_t s, int io = 0);
// three-launch path: partial forward / combine+filter / inverse
hipError_t launch_split_a(const DecimArgs& a, int nb, bool drop_in, hipStream_t s, int io = 0);
hipError_t launch_split_f(const DecimArgs& a, int nb, int mode, hipStream_t s);
hipError_t launch_split_b(const DecimArgs& a, int nb, bool drop_out, hipStream_t s, int io = 0);

// elementwise dropout for the plans without a fused epilogue (direct path): out = mask * scale * in
hipError_t launch_dropout_rows(const float* in, float* out, int B, long long row_elems, unsigned thr,
                               float scale, const unsigned long long* rng, hipStream_t s);
// saved = state; state[1] += 1      (one tiny launch: the generator advances on the device, so a captured
// hipGraph draws a fresh mask at every replay)
hipError_t launch_rng_next(unsigned long long* state, unsigned long long* saved, hipStream_t s);

// generic (any N, any k) kernels
struct DirectArgs {
  int B, N, D, F, k;    // k = number of bins of this launch
  const cf* tw;
  // bin i of the launch is frequency f0 + i * fstep (default: the first k bins)
  int f0 = 0, fstep = 1;
  // rows of the spectrum buffers: 0 = compact (B, k, D), row = i; otherwise (B, rows, D), row = frequency
  int rows = 0;
  int accumulate = 0;   // synthesis: y += instead of y =
  int R = 0;            // rows present in x / y (0 = N): zero-padded input, cropped output (Geom::R)
  __host__ __device__ int rows_present() const { return R ? R : N; }
};
hipError_t launch_direct_spectrum(const float* x, cf* xk, const DirectArgs& a, hipStream_t s);
hipError_t launch_direct_filter(const cf* xk, const float* w_re, const float* w_im, int conj_w,
                                cf* sk, const DirectArgs& a, hipStream_t s);
hipError_t launch_direct_synth(const cf* sk, const float* bias, float* y, const DirectArgs& a,
                               hipStream_t s);
hipError_t launch_scale_bins(const cf* in, cf* out, int B, int k, int D, int N, float scale, int hermitian,
                             hipStream_t s);
// large problems on the direct plan go through LDS-tiled kernels (k_tiled_spectrum / k_tiled_synth) inside
// the two launchers above; option "tiled_dft" = 0 keeps the literal fp64 kernels (A/B, tests)
void set_tiled_dft(int on);
// band-group edge bins: spectrum of the few bins f0 + i fstep with the rows spread over the grid;
// part = edge_chunks(B,N,D) * B * k * D * 2 doubles of scratch
int edge_chunks(int B, int N, int D);
hipError_t launch_edge_spectrum(const float* x, cf* xk, double* part, const DirectArgs& a,
                                hipStream_t s);
// y += the edge bins' part of the synthesis; sk compact (B, k, D), already scaled by 1/N
hipError_t launch_edge_synth_acc(const cf* sk, float* y, const DirectArgs& a, hipStream_t s);
// band-group edge bins (frequencies f0 + i fstep): products X conj(G) / N into the rows of the
// (B, k_total, D) grad slab, X from the saved spectrum (rows = frequency), G compact (B, k, D)
hipError_t launch_edge_slab(const cf* xk, const cf* ge, cf* slab, int k_total, const DirectArgs& a,
                            hipStream_t s);

// wt (k, D) complex <- (w_re, w_im) (D, F): the filter transposed and interleaved for the unpack phase
hipError_t launch_pack_w(const float* w_re, const float* w_im, cf* wt, int D, int F, int k,
                         hipStream_t s);

// parameter-gradient reductions (deterministic: fixed order over the batch)
hipError_t launch_gradw_slab(const cf* pslab, const float* gb_part, float* gw_re, float* gw_im,
                             float* gbias, int B, int D, int F, int k, hipStream_t s);
hipError_t launch_gradw_spectra(const cf* xk, const cf* gk, float* gw_re, float* gw_im,
                                float* gbias, int B, int N, int D, int F, int k, hipStream_t s);

// complex-in / complex-out filter of wirtinger_ops.WirtingerSpectralFilter and the x*w Function
hipError_t launch_wfilter(const cf* xf, const float* w_re, const float* w_im, int conj_w, cf* out,
                          int B, int N, int D, int F, int k, hipStream_t s);
hipError_t launch_wfilter_gradw(const cf* xf, const cf* gf, float* gw_re, float* gw_im, int B,
                                int N, int D, int F, int k, hipStream_t s);
hipError_t launch_cmul(const cf* x, const cf* w, int conj_w, cf* out, long long batch,
                       long long inner, hipStream_t s);
hipError_t launch_cmul_gradw(const cf* x, const cf* g, cf* gw, long long batch, long long inner,
                             hipStream_t s);

// ---- depthwise causal 3-tap convolution on (B, T, C): BicameralBlock's time path (smx_time.hip) ----------------------
size_t dwconv3_workspace_bytes(int B, int T, int C);        // partial sums of the backward: [B ceil(T/32)][5][C] floats
hipError_t launch_dwconv3_fwd(const float* x, const float* w, const float* bias, const float* scale, float* y, int B,
                              int T, int C, hipStream_t s);
hipError_t launch_dwconv3_bwd(const float* g, const float* x, const float* w, const float* bias, const float* scale,
                              float* gx, float* gw, float* gbias, float* gscale, float* part, int B, int T, int C,
                              hipStream_t s);

// ---- SpectralLayerNorm on a (B, F, C) complex spectrum, gamma / beta rows per bin (smx_time.hip) ----------------------
bool spectral_ln_supported(int C);         // C <= 1024: the row lives in one wavefront's registers
// planar: out / g are (2, B, F, C) float32 planes (real, imaginary) instead of interleaved complex
hipError_t launch_spectral_ln_fwd(const cf* z, const float* gamma, const float* beta, float eps, cf* out, int planar,
                                  int B, int F, int C, hipStream_t s);
hipError_t launch_spectral_ln_bwd(const cf* g, const cf* z, const float* gamma, const float* beta, float eps, cf* gz,
                                  float* ggamma, float* gbeta, int planar, int B, int F, int C, hipStream_t s);
// the planar side of SpectralFFN: complex factor per (bin, channel) on (2, B, F, C) planes; planar <-> interleaved
hipError_t launch_pcmul_fwd(const float* h, const float* fr, const float* fi, float* out, int B, int F, int C,
                            hipStream_t s);
hipError_t launch_pcmul_bwd(const float* g, const float* h, const float* fr, const float* fi, float* gh, float* gfr,
                            float* gfi, int B, int F, int C, hipStream_t s);
hipError_t launch_add_planar(const cf* a, const float* p, cf* y, long long n, hipStream_t s);   // y = a + (p0 + i p1)
hipError_t launch_to_planar(const cf* g, float* p, long long n, hipStream_t s);
// BicameralBlock's fusion line: out = r + w[0] a + w[1] b + c3 c  (smx_time.hip)
size_t mix_workspace_bytes();
hipError_t launch_mix_fwd(const float* r, const float* a, const float* b, const float* c, const float* w, float c3,
                          float* out, long long n, hipStream_t s);
hipError_t launch_mix_bwd(const float* g, const float* a, const float* b, const float* w, float c3, float* ga, float* gb,
                          float* gc, float* gw, float* part, long long n, hipStream_t s);
// the gate chain of the twin blocks: y = ((((x a[f]) u[c]) p[f]) q[b,c]) m[f]  (smx_time.hip)
size_t gate_workspace_bytes(int B, int F, int C);
hipError_t launch_gate_fwd(const cf* x, const cf* a, const float* u, const float* p, const float* q, const float* m, cf* y,
                           int B, int F, int C, hipStream_t s);
hipError_t launch_gate_bwd(const cf* g, const cf* x, const cf* a, const float* u, const float* p, const float* q,
                           const float* m, cf* gx, cf* s1, float* rc, float* rp, cf* part, int B, int F, int C,
                           hipStream_t s);

// ---- SpectralEMA scan, one lane per chain (b, f) (smx_ema.hip) -------------------------------------------------------
// kind 0: ptr = complex chunks (B, S, F); kind 1 / 2: ptr = uint8 / int64 tokens, rows row_stride elements apart,
// chunk t of row b = the L-point real DFT of tokens[b, t L : (t + 1) L] / 127.5 - 1, F = L / 2 + 1
struct EmaSrc { const void* ptr; int kind; long long row_stride; int B, S, F, L; };
size_t ema_states_bytes(int B, int S, int F);      // backward scratch: the pre-step states
size_t ema_part_bytes(int B, int F);               // backward scratch: per-chain parameter gradients
hipError_t launch_ema(const EmaSrc& src, bool polar, const cf* init, const float* rho_logit, const float* theta_raw,
                      cf* out, hipStream_t s);
hipError_t launch_ema_bwd(const EmaSrc& src, bool polar, const cf* g, const cf* init, const float* rho_logit,
                          const float* theta_raw, cf* gx, cf* ginit, float* g_rho, float* g_th, cf* states, float* part,
                          hipStream_t s);
// Word-structure targets of byte tokens (B, T), one workgroup per row: phase (B, T, 2) and / or boundary (B, T), either
// may be null.  kind 1 / 2: uint8 / int64 tokens, rows row_stride elements apart.  T <= WT_MAX_T.
constexpr int WT_MAX_T = 65536;
constexpr int WT_BLOCK = 256;            // threads per row; thread i owns the 64-position words [i WPT, (i + 1) WPT)
hipError_t launch_word_targets(const void* tokens, int kind, long long row_stride, float* phase, float* boundary, int B,
                               int T, hipStream_t s);

// ---- LayerNorm row kernels of the fused block (smx_block.hip) -------------------------------------
constexpr int ROW_WAVES = 4;             // wavefronts (rows in flight) per block of the kernels sized by ln_num_blocks
constexpr int LN_MAX_BLOCKS = 2048;      // most rows of the grad_gamma / grad_beta partial buffer
int ln_num_blocks(long long rows);       // blocks (= partial rows) a backward launch uses for `rows` rows, ROW_WAVES each
constexpr int LN_MAX_D = 4096;           // widest row held in registers (D % 4 == 0)
constexpr int LN_MAX_D_ODD = 1024;       // same for the scalar variant (D % 4 != 0)
bool ln_supported(int D);
hipError_t launch_ln_stats(const float* x, cf* stats, long long rows, int D, float eps,
                           hipStream_t s);
hipError_t launch_ln_apply(const float* x, const cf* stats, const float* gamma, const float* beta,
                           float* h, long long rows, int D, hipStream_t s);
hipError_t launch_add_rows(float* y, const float* x, size_t total, hipStream_t s);
// in place over grad_h; part: (ln_num_blocks(rows), 2, D) floats of scratch
hipError_t launch_ln_bwd(float* gh_dx, const float* x, const float* g, const cf* stats,
                         const float* gamma, float* part, float* g_gamma, float* g_beta,
                         long long rows, int D, hipStream_t s);
// g_gamma[d] = sum_blk part[blk][0][d], g_beta[d] = sum_blk part[blk][1][d] (fixed order; either may be null)
// 2-byte rows (io = SMX_IO_BF16 / SMX_IO_F16; D % 4 == 0): x, g, dx in the io type, gh (B, N, D) f32 read-only, dx != gh
bool ln_io_supported(int D);
hipError_t launch_ln_stats_io(const void* x, cf* stats, long long rows, int D, float eps, hipStream_t s, int io);
hipError_t launch_ln_bwd_io(const float* gh, const void* x, const void* g, void* dx, const cf* stats,
                            const float* gamma, float* part, float* g_gamma, float* g_beta, long long rows, int D,
                            hipStream_t s, int io);
hipError_t launch_ln_colsum(const float* part, int nblk, int D, float* g_gamma, float* g_beta, hipStream_t s);
// The O-neuron head (O = 1, 2) over R rows of width C (ln_supported(C)): y[r, o] = sum_e h[r, e] w[o, e] + b[o].
// Backward: grad_h = g w; block partials of grad_w in part_w (ln_num_blocks(R), 2, C) and of grad_b in part_b
// (ln_num_blocks(R), 2), both reduced by k_ln_colsum in a fixed order.  Each of grad_h / grad_w / grad_b may be null.
size_t head_part_w_bytes(long long R, int C);
size_t head_part_b_bytes(long long R);
hipError_t launch_head_fwd(const float* h, const float* w, const float* b, float* y, long long R, int C, int O,
                           hipStream_t s);
hipError_t launch_head_bwd(const float* g, const float* h, const float* w, float* grad_h, float* grad_w, float* grad_b,
                           float* part_w, float* part_b, long long R, int C, int O, hipStream_t s);
// Softmax cross-entropy over R rows of V fp32 logits, rows row_stride elements apart, int64 targets (reference
// fft_lm/dual_head.py:176-188).  Forward: lse[r] = (m, d) = (max_j x[r, j], log sum_j exp(x[r, j] - m)), a pair of floats
// whose sum is the row's log-sum-exp, the row loss d - (x[r, t_r] - m) (into loss_rows when reduction is XENT_NONE), one (sum, count) partial per block in part (xent_num_blocks(R) pairs), then one
// workgroup adds the partials in index order into loss[0] (mean / sum) and count[0].  Backward: grad (R, V) dense =
// (exp((x - m) - d) - [j == t]) s_r, s_r from g and count in device memory.  A row whose target is ignore_index is not read:
// its loss, lse and gradient row are zeros.  A target outside [0, V) makes its row's loss and gradient NaN.
// Register rows (one wavefront a row) for ln_supported(V), as Vec<4> only where logits, grad and row_stride keep every
// row 16-byte aligned; streaming rows (one workgroup a row, any alignment) for every other V.
constexpr int XENT_MEAN = 0, XENT_SUM = 1, XENT_NONE = 2;
constexpr int XENT_BLOCK = 256;          // threads of a streaming row's workgroup and of the finishing workgroup
int xent_num_blocks(long long R);        // most (sum, count) partials either family writes for R rows
hipError_t launch_xent_fwd(const float* logits, long long row_stride, const long long* targets, long long ignore_index,
                           int reduction, float* loss, float* lse, float* count, float* part, long long R, int V,
                           hipStream_t s);
hipError_t launch_xent_bwd(const float* g, const float* logits, long long row_stride, const long long* targets,
                           long long ignore_index, int reduction, const float* lse, const float* count, float* grad,
                           long long R, int V, hipStream_t s);

// ---- row kernels of EnhancedSpectralBlock (smx_enh.hip) --------------------------------------------
constexpr int ENH_MAX_D = 1024;          // widest row (even) held in one wavefront's registers; the gate row is 2D
bool enh_supported(int D);
// partial-sum scratch of the backward launches: ln_num_blocks(rows) x 4 x D floats
size_t enh_part_floats(long long rows, int D);
// A: x1 = x + M1 rot(LN1(x)), h2 = LN2(x1), stats (2, B T) (mean, rstd) of both norms; norm == false: x1 = rot(x)
hipError_t launch_rope_fwd(const float* x, const float* rot, const float* w1, const float* b1, const float* w2,
                           const float* b2, float eps1, float eps2, float* x1, float* h2, cf* stats, int B, int T,
                           int D, bool norm, unsigned thr, float scale, const unsigned long long* rng, hipStream_t s);
hipError_t launch_rope_bwd(const float* g1, const float* gh2, const float* x, const float* rot, const float* w1,
                           const float* b1, const float* w2, const cf* stats, float* gx, float* gw1, float* gb1,
                           float* gw2, float* gb2, float* part, int B, int T, int D, bool norm, unsigned thr,
                           float scale, const unsigned long long* rng, hipStream_t s);
// B: x2 = x1 + M2 p, h3 = LN3(x2)
hipError_t launch_res_fwd(const float* x1, const float* p, const float* w3, const float* b3, float eps, float* x2,
                          float* h3, cf* stats, int B, int T, int D, unsigned thr, float scale,
                          const unsigned long long* rng, hipStream_t s);
hipError_t launch_res_bwd(const float* g2, const float* gh3, const float* x2, const float* w3, const cf* stats,
                          float* gx1, float* gp, float* gw3, float* gb3, float* part, int B, int T, int D, unsigned thr,
                          float scale, const unsigned long long* rng, hipStream_t s);
// C: x3 = x2 + M3 (gate v + (1 - gate) vt), [gate pre-activation | vt] = LN_2D(a); x2 may be null
hipError_t launch_gate_blend_fwd(const float* a, const float* v, const float* x2, const float* wg, const float* bg,
                                 float eps, float* x3, cf* stats, int B, int T, int D, unsigned thr, float scale,
                                 const unsigned long long* rng, hipStream_t s);
hipError_t launch_gate_blend_bwd(const float* g3, const float* a, const float* v, const float* wg, const float* bg,
                                 const cf* stats, float* ga, float* gv, float* gwg, float* gbg, float* part, int B,
                                 int T, int D, unsigned thr, float scale, const unsigned long long* rng,
                                 hipStream_t s);

// ---- overlap-save chunk generation: the window ring of a FixedSpectralBlock (smx_stream.hip) -----------------
constexpr int STREAM_MAX_K = 4096;       // longest kernel, and with it the tap table held in LDS
constexpr int STREAM_MAX_CHUNK = 64;
bool stream_supported(int T, int K, int C, int chunk);
// ring[b, (pos[b] + n) % T] = LN(h[b, n]), (hi, lo) += new - evicted, pooled = (hi + lo) / T, pos += chunk
hipError_t launch_stream_push(const float* h, const float* ln_w, const float* ln_b, float eps, float* ring, float* sum,
                              int* pos, float* pooled, int Bt, int T, int C, int chunk, hipStream_t s);
// h_out = h + scale * (Toeplitz slice of taps) (last K - 1 + chunk ring rows), ff_in = LN(h_out) (nullable)
hipError_t launch_stream_conv(const float* h, const float* ring, const int* pos, const float* taps, const float* scale,
                              const float* ln_w, const float* ln_b, float eps, float* h_out, float* ff_in, int Bt, int T,
                              int K, int C, int chunk, hipStream_t s);

// ---- the byte sampler of generation (smx_stream.hip, k_sample_bytes) ------------------------------------------
constexpr int SAMPLE_V = 256;            // the vocabulary: one thread per byte
constexpr int SAMPLE_MAX_RECENT = 65536;
struct SampleArgs {
  float temperature, top_p, rep, presence, frequency;
  int top_k, ascii_only, ban_cr, max_run;
};
// ids[r] (and probs[r, :], nullable) of R rows of SAMPLE_V logits, row_stride floats apart; recent: n_recent ids shared
// by the rows, kind 1 / 2 = uint8 / int64; u (R) uniforms in [0, 1).  One workgroup per row.
hipError_t launch_sample_bytes(const float* logits, long long row_stride, const void* recent, int kind, int n_recent,
                               const SampleArgs& a, const float* u, long long* ids, float* probs, long long R,
                               hipStream_t s);

// ---- steps the units below share ----------------------------------------------------------------------------------------
// a workspace part: rounded up to 256 bytes
inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
// Persistent workgroups that walk `ntiles` tiles g, g + G, ...: as many as stay resident (`cap`; `max_workgroups` > 0
// lowers it: tests force the walk with 1 or 2), cut down so that every workgroup walks the same number of tiles, give or
// take one.  No tiles: none.
inline int tile_workgroups(long long ntiles, long long cap, int max_workgroups) {
  if (ntiles <= 0) return 0;
  if (max_workgroups > 0 && max_workgroups < cap) cap = max_workgroups;
  const long long rounds = (ntiles + cap - 1) / cap;
  return (int)((ntiles + rounds - 1) / rounds);
}

// ---- byte-spectral features (smx_byte.hip) ----------------------------------------------------------------------------
struct ByteArgs {
  const void* tokens;
  long long row_stride;
  const float* bands;
  float* out;
  float* mag;
  int B, T, k, W, P;
  int pp, chunks;                  // positions per workgroup, workgroups per batch row
  int ns_log;                      // lanes per bin = 1 << ns_log (<= 64)
  int cw_log;                      // threads across a row = 1 << cw_log
};
bool byte_supported(int T, int k, int W);
// out (B, P, W), mag (B, k; nullable) of tokens (B, T), kind 1 / 2 = uint8 / int64, rows row_stride elements apart; P = 1 or
// T.  Derives pp, chunks, ns_log, cw_log.
hipError_t launch_byte_features(const void* tokens, int kind, long long row_stride, const float* bands, float* out,
                                float* mag, int B, int T, int k, int W, int P, hipStream_t s);
// grad_bands (n_bands) from g (B, P, W) and mag (B, k) over kk = min(k, W) columns: per-chunk partials in `part`
// (byte_gb_part_bytes; untouched when kk = 0), then their sum.  byte_gb_blocks: workgroups of the partial launch.
long long byte_gb_blocks(int B, int P, int kk);
size_t byte_gb_part_bytes(int B, int P, int kk);
hipError_t launch_byte_grad_bands(const float* g, const float* mag, float* part, float* grad_bands, int n_bands, int B,
                                  int P, int W, int k, hipStream_t s);

// ---- multi-pattern exact byte search (smx_match.hip) ------------------------------------------------------------------
struct MatchArgs {
  const unsigned char* corpus;
  const unsigned char* snips;
  unsigned long long* part;        // (G, S)
  long long n;                     // corpus bytes
  long long npos;                  // n - L + 1 > 0
  long long ntiles;
  int S, L, off, nvec;             // nvec: 16-byte vectors of a tile's image, ceil((TILE + L - 1) / 16)
};
bool match_supported(int S, int L);
size_t match_part_bytes(int S);          // the (workgroups, S) table of minima
// first[s] of S snippets of L bytes in corpus[0 : n]; derives off, nvec, npos, ntiles and the workgroups from the LDS of
// (S, L); n < L: the join alone
hipError_t launch_match_first(const unsigned char* corpus, long long n, const unsigned char* snips, int S, int L,
                              long long* first, unsigned long long* part, int max_workgroups, hipStream_t s);

// ---- top-k sparsify and scatter of the sparse spectral tensor (smx_sst.hip) ------------------------------------------------
struct TopkState {                                        // written by k_topk_pick, read by the next pass
  unsigned prefix;                                        // the key bits decided so far (right-aligned)
  unsigned rank;                                          // the rank of T among the keys that share the prefix (1-based)
  unsigned above;                                         // keys greater than every key that shares the prefix
  unsigned pad;
};

struct TopkArgs {
  const float2* z;
  long long n;
  long long ntiles;
  int off;                                                // 0 or 1: elements between the 16-byte boundary below z and z
};
bool topk_supported(long long n);
// workspace of select / compact: TopkState at 0, then the offsets of the column totals, the histogram rows and the tile
// counts (after select: offsets); need: its size
struct TopkLayout { size_t totals, rows, counts, need; };
TopkLayout topk_layout(long long n);
hipError_t launch_topk_select(const float2* z, long long n, long long k, long long* result, void* workspace,
                              int max_workgroups, hipStream_t s);
hipError_t launch_topk_compact(const float2* z, long long n, const long long* result, float2* coeffs, long long* flat_idx,
                               long long capacity, const void* workspace, int max_workgroups, hipStream_t s);
hipError_t launch_sparse_scatter(const float2* coeffs, const long long* flat_idx, long long m, float2* out, long long n,
                                 int max_workgroups, hipStream_t s);

// ---- frequency attention and frequency layernorm (smx_freq.hip) ---------------------------------------------------------
struct FattnArgs {
  const float2* q;
  const float2* k;
  const float2* v;
  float2* out;
  long long sq[3], sk[3], sv[3], so[3];   // element strides of the b, h and n axes; the innermost axis is contiguous
  long long rows;                         // B H N
  int H, N, D;
  float scale;                            // 1 / (temperature D)
};
constexpr int FATTN_MAX_N = 1 << 30;
constexpr int FATTN_MAX_WG = 2048;        // workgroups of k_fattn_apply above which its tiles grow past 64 rows
int fattn_tile_rows(long long BH, int N);
constexpr int FREQ_LN_MAX_D = 1024;       // widest complex row held in registers (SMX_FREQ_LN_MAX_D of smx_freq.h)
inline bool freq_ln_supported(int D) { return D >= 1 && D <= FREQ_LN_MAX_D; }
// The two launchers are WEAK references: a link that lists its units itself and leaves smx_freq out (the host-only
// program of tests/api_trace) still resolves smx_api's entries, which refuse with SMX_ERR_UNSUPPORTED where a launcher is
// absent.  libsmx.so always holds them (csrc/build.sh).
// scores: B H N floats of scratch.  Two launches (scores; statistics + apply).
__attribute__((weak)) hipError_t launch_fattn(const FattnArgs& a, float* scores, hipStream_t s);
// z, out: (rows, D) complex64 dense, 16-byte aligned
__attribute__((weak)) hipError_t launch_freq_ln(const float* z, float* out, float eps, long long rows, int D, hipStream_t s);

// ---- per-bin channel contraction of the FFT convolutions (smx_fconv.hip) ----------------------------------------------------
// x (B, P, Ci), w (P, Ci, Co), y / gy (B, P, Co), all complex64, dense, 8-byte aligned.  WEAK references like the two
// above, for the same reason; smx_api's entries answer through the launchers alone, so the size rule is weak too.
__attribute__((weak)) bool bin_contract_supported(int B, long long P, int Ci, int Co);
// y[b, p, o] = sum_i x[b, p, i] w[p, i, o].  One launch.
__attribute__((weak)) hipError_t launch_bin_contract_fwd(const float2* x, const float2* w, float2* y, int B, long long P, int Ci,
                                                         int Co, int max_workgroups, hipStream_t s);
// gx[b, p, i] = sum_o gy conj(w) (needs w), gw[p, i, o] = sum_b conj(x) gy (needs x); either may be NULL: a launch each.
__attribute__((weak)) hipError_t launch_bin_contract_bwd(const float2* x, const float2* w, const float2* gy, float2* gx,
                                                         float2* gw, int B, long long P, int Ci, int Co, int max_workgroups,
                                                         hipStream_t s);

// ---- the polar and log8 codecs of the compressed spectra (smx_quant.hip) -----------------------------------------------------
// z complex64 (8-byte aligned), x fp32, the code planes uint8 at any byte address; n > 0.  WEAK references like the ones
// above, for the same reason.
__attribute__((weak)) size_t quant_range_part_bytes();
// out2 = (min, max) over the elements of log2(max(|z|, 1e-9)); part: quant_range_part_bytes().  Two launches.
__attribute__((weak)) hipError_t launch_polar_range(const float2* z, long long n, float* out2, float2* part,
                                                    int max_workgroups, hipStream_t s);
__attribute__((weak)) hipError_t launch_polar_quantize(const float2* z, unsigned char* mag_q, unsigned char* phase_q,
                                                       long long n, int mag_bits, int phase_bits, float mag_min,
                                                       float mag_max, int max_workgroups, hipStream_t s);
__attribute__((weak)) hipError_t launch_polar_dequantize(const unsigned char* mag_q, const unsigned char* phase_q, float2* z,
                                                         long long n, int mag_bits, int phase_bits, float mag_min,
                                                         float mag_max, int max_workgroups, hipStream_t s);
__attribute__((weak)) hipError_t launch_log8_encode(const float* x, unsigned char* e, long long n, int max_workgroups,
                                                    hipStream_t s);
__attribute__((weak)) hipError_t launch_log8_decode(const unsigned char* e, float* x, long long n, int max_workgroups,
                                                    hipStream_t s);
__attribute__((weak)) hipError_t launch_log8_encode_c64(const float2* z, unsigned char* re_q, unsigned char* im_q, long long n,
                                                        int max_workgroups, hipStream_t s);
__attribute__((weak)) hipError_t launch_log8_decode_c64(const unsigned char* re_q, const unsigned char* im_q, float2* z,
                                                        long long n, int max_workgroups, hipStream_t s);

// ---- the DFT along the contiguous last axis of dense rows (smx_rowfft.hip) ---------------------------------------------------
// n: a power of two from 2 to 4096 (SMX_ROWFFT_MAX_N)
inline bool rowfft_supported(int n) { return n >= 2 && n <= 4096 && (n & (n - 1)) == 0; }
// in / out: (rows, n) complex64, or fp32 on the side that flags (SMX_ROWFFT_*) marks real; 16-byte aligned; rows > 0.  One
// launch.  A WEAK reference like the ones above, for the same reason.
__attribute__((weak)) hipError_t launch_rowfft(const void* in, void* out, long long rows, int n, int flags, float scale,
                                               int max_workgroups, hipStream_t s);

}  // namespace smx
