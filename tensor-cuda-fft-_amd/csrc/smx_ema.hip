// smx_ema.hip -- SpectralEMA: the frequency-domain state-space memory of fft_lm's chunk head
// (reference fft_lm/spectral_ssm.py:71-125, its caller fft_lm/chunk_head.py:53-66) as ONE scan launch.
//
// The reference steps a (B, F) complex state through S chunks with about fifteen small elementwise ops per step.
// Its aligned step `state * exp(i (angle(X) - angle(state)))` is |state| u(X) with u(X) = X / |X| (u = 1 at X == 0,
// because angle(0) = 0), so with rho = sigmoid(rho_logit), theta = pi tanh(theta_raw), a = rho e^{i theta}:
//     aligned:  H' = a |H| u(X) + (1 - rho) X
//     polar:    H' = (rho |H| + (1 - rho) |X|) u(X)
// The recurrence is nonlinear in H (it uses |H|): no associative scan, no FFT.  Every chain (b, f) is sequential and
// all chains are independent: one lane per chain, chains flattened over (b, f) so that F = 9 still fills wavefronts
// and the loads of chunks[b, t, :] stay contiguous along f.  What a step reads does not depend on the state, so it
// is fetched EMA_PF steps ahead of the dependent chain (|H| -> one fma per component).
//
// Backward: one launch.  Each lane reruns its forward chain, leaving the pre-step states in the caller's workspace
// (B, S, F complex, written and read back by the same lane), then walks t in reverse.  The parameter gradients are
// summed per chain in registers, stored as per-chain partials, and a second small launch adds them over the batch in
// a fixed order (bitwise reproducible; no atomics, no flags, no spin-waits).
//
// Token front end: the same two bodies behind a loader that forms chunk t of row b from byte tokens on the fly,
// x = byte / 127.5 - 1 = (2 byte - 255) / 255, bin f of the L-point real DFT (reference chunk_head.py:60-63) as a direct
// sum over a twiddle table in LDS: the (B, S, F) spectrum never exists in memory.  The sums run over the INTEGERS
// 2 byte - 255 (minus the chunk's first one for f > 0, which changes nothing because the twiddles of a bin f > 0
// sum to zero): the DC and Nyquist bins are exact integer sums, and a run of equal bytes gives an exact zero in every
// bin f > 0 -- where the kernel then takes u = 1.
//
// Also here, because the byte-token loader is: k_word_targets, the word-structure targets of the same tokens (phase
// clock and boundary labels of fft_lm/phase_clock.py, fft_lm/segmentation_head.py) as one launch.
#include "smx_kernels.h"

namespace smx {

constexpr int EMA_PF = 4;          // steps fetched ahead of the dependent chain
constexpr int EMA_BLOCK = 64;      // one wavefront per workgroup: the chains are latency-bound, spread them over the CUs

struct EmaCoef {
  float rho, c;                    // rho, 1 - rho
  float er, ei;                    // e^{i theta}
  float drho, dth;                 // d rho / d rho_logit, d theta / d theta_raw
};

SMX_HD EmaCoef ema_coef(float rho_logit, float theta_raw, bool polar) {
  EmaCoef k;
  k.rho = 1.f / (1.f + expf(-rho_logit));
  k.c = 1.f - k.rho;
  k.drho = k.rho * k.c;
  k.er = 1.f; k.ei = 0.f; k.dth = 0.f;
  if (!polar) {
    const float th = tanhf(theta_raw);
#if defined(__HIP_DEVICE_COMPILE__)
    sincospif(th, &k.ei, &k.er);
#else
    k.ei = sinf(3.14159265358979323846f * th); k.er = cosf(3.14159265358979323846f * th);   // host pass: never run
#endif
    k.dth = 3.14159265358979323846f * (1.f - th * th);
  }
  return k;
}

// |z| and z / |z| through a power-of-two scaling of both components (exact), so that neither x^2 + y^2 nor
// 1 / |z| overflows or flushes anywhere in the fp32 range; z == 0 -> r = 0, u = 1 (angle(0) = 0).
SMX_HD void ema_polar(cf z, float* r, cf* u) {
  const float s = fmaxf(fabsf(z.x), fabsf(z.y));
  if (s == 0.f) { *r = 0.f; *u = mk(1.f, 0.f); return; }
  int e;
  (void)frexpf(s, &e);
  const float xs = ldexpf(z.x, -e), ys = ldexpf(z.y, -e);
  const float rs = sqrtf(xs * xs + ys * ys), inv = 1.f / rs;
  *r = ldexpf(rs, e);
  *u = mk(xs * inv, ys * inv);
}
SMX_HD float ema_abs(cf z) {
  const float s = fmaxf(fabsf(z.x), fabsf(z.y));
  if (s == 0.f) return 0.f;
  int e;
  (void)frexpf(s, &e);
  const float xs = ldexpf(z.x, -e), ys = ldexpf(z.y, -e);
  return ldexpf(sqrtf(xs * xs + ys * ys), e);
}

// What a step needs of its chunk, formed off the dependent chain.
//   aligned: H' = |H| w + cx     polar: H' = (rho |H| + cr) u
struct EmaIn { cf w, cx; };
template <bool POLAR>
SMX_HD EmaIn ema_in(const EmaCoef& k, cf X) {
  float r; cf u;
  ema_polar(X, &r, &u);
  EmaIn in;
  if (POLAR) { in.w = u; in.cx = mk(k.c * r, 0.f); }
  else {
    in.w = mk(k.rho * (k.er * u.x - k.ei * u.y), k.rho * (k.er * u.y + k.ei * u.x));
    in.cx = mk(k.c * X.x, k.c * X.y);
  }
  return in;
}
template <bool POLAR>
SMX_HD cf ema_step(const EmaCoef& k, cf H, const EmaIn& in) {
  const float m = ema_abs(H);
  if (POLAR) { const float M = k.rho * m + in.cx.x; return mk(M * in.w.x, M * in.w.y); }
  return mk(m * in.w.x + in.cx.x, m * in.w.y + in.cx.y);
}

// ---- loaders: chunk t of one chain ----------------------------------------------------------------------------------
struct ChunkLoader {
  const cf* base;                  // chunks + b S F + f
  size_t stride;                   // F
  SMX_HD cf operator()(int t) const { return base[(size_t)t * stride]; }
};
// tw[j] = (cos, sin)(2 pi j / L); X_f = sum_n x_n e^{-2 pi i f n / L}
template <typename TOK>
struct TokenLoader {
  const TOK* row;                  // tokens + b row_stride
  const cf* tw;
  int L, f;
  SMX_HD cf operator()(int t) const {
    const TOK* p = row + (size_t)t * L;
    const int base = f ? 2 * (int)p[0] - 255 : 0;
    float re = 0.f, im = 0.f;
    int j = 0;
    for (int n = 0; n < L; ++n) {
      const float d = (float)(2 * (int)p[n] - 255 - base);
      const cf w = tw[j];
      re = fmaf(d, w.x, re);
      im = fmaf(d, w.y, im);
      j += f;
      if (j >= L) j -= L;
    }
    constexpr float SC = 1.f / 255.f;
    return mk(re * SC, -im * SC);
  }
};

// ---- the two chain bodies -------------------------------------------------------------------------------------------
// Forward chain from H; save != nullptr: the pre-step state of step t goes to save[t stride].
template <bool POLAR, class LD>
SMX_HD cf ema_chain_fwd(const LD& ld, const EmaCoef& k, cf H, int S, cf* save, size_t stride) {
  cf q[EMA_PF];
#pragma unroll
  for (int j = 0; j < EMA_PF; ++j) q[j] = j < S ? ld(j) : mk(0.f, 0.f);
  for (int t0 = 0; t0 < S; t0 += EMA_PF) {
#pragma unroll
    for (int j = 0; j < EMA_PF; ++j) {
      const int t = t0 + j;
      if (t < S) {
        const EmaIn in = ema_in<POLAR>(k, q[j]);
        if (t + EMA_PF < S) q[j] = ld(t + EMA_PF);
        if (save) save[(size_t)t * stride] = H;
        H = ema_step<POLAR>(k, H, in);
      }
    }
  }
  return H;
}

// Reverse walk over the saved pre-step states.  G: gradient of the final state on entry, of the initial state on
// return.  gx (nullable): gradient of chunk t at gx[t stride].  acc: d L / d rho, d L / d theta of this chain.
// With q = conj(e^{i theta} u) G:
//   aligned: dL/d|H| = rho Re q; at H == 0 the reference's autograd hands conj(a u) G = rho q to the state instead
//            (angle's gradient is 0 there); grad X = c G + (|H| rho Im q / |X|) i u;
//            dL/drho = |H| Re q - Re(conj(X) G); dL/dtheta = |H| rho Im q.
//   polar (q = conj(u) G, M = rho |H| + c |X|): grad H = rho Re q H / |H| (0 at H == 0);
//            grad X = (c Re q) u + (M Im q / |X|) i u (0 at X == 0); dL/drho = Re q (|H| - |X|).
template <bool POLAR, class LD>
SMX_HD cf ema_chain_bwd(const LD& ld, const EmaCoef& k, cf G, int S, const cf* saved, cf* gx, size_t stride,
                        float* acc_rho, float* acc_th) {
  cf qx[EMA_PF], qh[EMA_PF];
#pragma unroll
  for (int j = 0; j < EMA_PF; ++j) {
    qx[j] = j < S ? ld(S - 1 - j) : mk(0.f, 0.f);
    qh[j] = j < S ? saved[(size_t)(S - 1 - j) * stride] : mk(0.f, 0.f);
  }
  float a_rho = 0.f, a_th = 0.f;
  for (int i0 = 0; i0 < S; i0 += EMA_PF) {
#pragma unroll
    for (int j = 0; j < EMA_PF; ++j) {
      const int i = i0 + j;
      if (i < S) {
        const int t = S - 1 - i;
        const cf X = qx[j], H = qh[j];
        if (i + EMA_PF < S) {
          qx[j] = ld(t - EMA_PF);
          qh[j] = saved[(size_t)(t - EMA_PF) * stride];
        }
        float r, m; cf u, v;
        ema_polar(X, &r, &u);
        ema_polar(H, &m, &v);                       // v = H / |H| (unused at H == 0)
        const float inv_r = r > 0.f ? 1.f / r : 0.f; // X == 0: angle's and abs's gradients are 0
        cf gX, gH;
        if (POLAR) {
          const float qr = u.x * G.x + u.y * G.y, qi = u.x * G.y - u.y * G.x;
          const float M = k.rho * m + k.c * r;
          const float rad = r > 0.f ? k.c * qr : 0.f, tan = M * qi * inv_r;
          gX = mk(rad * u.x - tan * u.y, rad * u.y + tan * u.x);
          const float gm = m > 0.f ? k.rho * qr : 0.f;
          gH = mk(gm * v.x, gm * v.y);
          a_rho += qr * (m - r);
        } else {
          const cf eu = mk(k.er * u.x - k.ei * u.y, k.er * u.y + k.ei * u.x);
          const float qr = eu.x * G.x + eu.y * G.y, qi = eu.x * G.y - eu.y * G.x;
          const float tan = m * k.rho * qi * inv_r;
          gX = mk(k.c * G.x - tan * u.y, k.c * G.y + tan * u.x);
          if (m > 0.f) { const float gm = k.rho * qr; gH = mk(gm * v.x, gm * v.y); }
          else gH = mk(k.rho * qr, k.rho * qi);
          a_rho += m * qr - (X.x * G.x + X.y * G.y);
          a_th += m * k.rho * qi;
        }
        if (gx) gx[(size_t)t * stride] = gX;
        G = gH;
      }
    }
  }
  *acc_rho = a_rho;
  *acc_th = a_th;
  return G;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------
struct EmaArgs {
  const void* src;                 // chunks (B, S, F) complex, or tokens
  long long tok_stride;            // tokens: elements between batch rows
  const cf* init;                  // (B, F) or null
  const float* rho_logit;          // (F)
  const float* theta_raw;          // (F); unused in polar mode
  cf* out;                         // forward: final state (B, F)
  const cf* g;                     // backward: gradient of the final state
  cf* gx;                          // (B, S, F) or null
  cf* ginit;                       // (B, F) or null
  cf* states;                      // workspace: pre-step states (B, S, F)
  float* part;                     // workspace: (2, B F) per-chain parameter gradients
  int B, S, F, L;
};

// SRC: 0 complex chunks, 1 uint8 tokens, 2 int64 tokens
template <int SRC> struct EmaTok { typedef unsigned char type; };
template <> struct EmaTok<2> { typedef long long type; };

template <int SRC>
__device__ __forceinline__ void ema_table(cf* tw, int L) {
  if (SRC != 0) {
    if ((int)threadIdx.x < L) {
      double s, c;
      sincospi((double)(2 * (int)threadIdx.x) / (double)L, &s, &c);   // exact at the multiples of a quarter turn
      tw[threadIdx.x] = mk((float)c, (float)s);
    }
    __syncthreads();
  }
}

template <int SRC, bool POLAR>
__global__ __launch_bounds__(EMA_BLOCK) void k_ema_fwd(EmaArgs a) {
  __shared__ cf tw[64];
  ema_table<SRC>(tw, a.L);
  const long long c = (long long)blockIdx.x * EMA_BLOCK + threadIdx.x;
  if (c >= (long long)a.B * a.F) return;
  const int b = (int)(c / a.F), f = (int)(c % a.F);
  const EmaCoef k = ema_coef(a.rho_logit[f], POLAR ? 0.f : a.theta_raw[f], POLAR);
  const cf H0 = a.init ? a.init[c] : mk(0.f, 0.f);
  cf H;
  if constexpr (SRC == 0) {
    const ChunkLoader ld{(const cf*)a.src + (size_t)b * a.S * a.F + f, (size_t)a.F};
    H = ema_chain_fwd<POLAR>(ld, k, H0, a.S, nullptr, 0);
  } else {
    typedef typename EmaTok<SRC>::type TOK;
    const TokenLoader<TOK> ld{(const TOK*)a.src + (size_t)b * a.tok_stride, tw, a.L, f};
    H = ema_chain_fwd<POLAR>(ld, k, H0, a.S, nullptr, 0);
  }
  a.out[c] = H;
}

template <int SRC, bool POLAR>
__global__ __launch_bounds__(EMA_BLOCK) void k_ema_bwd(EmaArgs a) {
  __shared__ cf tw[64];
  ema_table<SRC>(tw, a.L);
  const long long c = (long long)blockIdx.x * EMA_BLOCK + threadIdx.x;
  const long long BF = (long long)a.B * a.F;
  if (c >= BF) return;
  const int b = (int)(c / a.F), f = (int)(c % a.F);
  const EmaCoef k = ema_coef(a.rho_logit[f], POLAR ? 0.f : a.theta_raw[f], POLAR);
  const cf H0 = a.init ? a.init[c] : mk(0.f, 0.f);
  const size_t off = (size_t)b * a.S * a.F + f, st = (size_t)a.F;
  cf* saved = a.states + off;
  cf* gx = a.gx ? a.gx + off : nullptr;
  float a_rho, a_th;
  cf G;
  if constexpr (SRC == 0) {
    const ChunkLoader ld{(const cf*)a.src + off, st};
    (void)ema_chain_fwd<POLAR>(ld, k, H0, a.S, saved, st);
    G = ema_chain_bwd<POLAR>(ld, k, a.g[c], a.S, saved, gx, st, &a_rho, &a_th);
  } else {
    typedef typename EmaTok<SRC>::type TOK;
    const TokenLoader<TOK> ld{(const TOK*)a.src + (size_t)b * a.tok_stride, tw, a.L, f};
    (void)ema_chain_fwd<POLAR>(ld, k, H0, a.S, saved, st);
    G = ema_chain_bwd<POLAR>(ld, k, a.g[c], a.S, saved, nullptr, st, &a_rho, &a_th);
  }
  if (a.ginit) a.ginit[c] = G;
  if (a.part) {
    a.part[c] = a_rho * k.drho;
    a.part[BF + c] = a_th * k.dth;
  }
}

// grad_rho_logit[f] = sum_b part[0][b F + f], grad_theta_raw[f] = sum_b part[1][b F + f], b ascending
__global__ __launch_bounds__(EMA_BLOCK) void k_ema_param_sum(const float* __restrict__ part, float* __restrict__ g_rho,
                                                             float* __restrict__ g_th, int B, int F) {
  const int f = blockIdx.x * EMA_BLOCK + threadIdx.x;
  if (f >= F) return;
  const size_t BF = (size_t)B * F;
  float s0 = 0.f, s1 = 0.f;
  for (int b = 0; b < B; ++b) {
    s0 += part[(size_t)b * F + f];
    s1 += part[BF + (size_t)b * F + f];
  }
  if (g_rho) g_rho[f] = s0;
  if (g_th) g_th[f] = s1;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
size_t ema_states_bytes(int B, int S, int F) { return (size_t)B * S * F * sizeof(cf); }
size_t ema_part_bytes(int B, int F) { return (size_t)2 * B * F * sizeof(float); }

namespace {
template <int SRC>
void ema_launch(bool bwd, bool polar, const EmaArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)(((long long)a.B * a.F + EMA_BLOCK - 1) / EMA_BLOCK)), block(EMA_BLOCK);
  if (!bwd) {
    if (polar) hipLaunchKernelGGL((k_ema_fwd<SRC, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_ema_fwd<SRC, false>), grid, block, 0, s, a);
  } else {
    if (polar) hipLaunchKernelGGL((k_ema_bwd<SRC, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_ema_bwd<SRC, false>), grid, block, 0, s, a);
  }
}
}  // namespace

hipError_t launch_ema(const EmaSrc& src, bool polar, const cf* init, const float* rho_logit, const float* theta_raw,
                      cf* out, hipStream_t s) {
  EmaArgs a{};
  a.src = src.ptr; a.tok_stride = src.row_stride; a.init = init; a.rho_logit = rho_logit; a.theta_raw = theta_raw;
  a.out = out; a.B = src.B; a.S = src.S; a.F = src.F; a.L = src.L;
  if (src.kind == 0) ema_launch<0>(false, polar, a, s);
  else if (src.kind == 1) ema_launch<1>(false, polar, a, s);
  else ema_launch<2>(false, polar, a, s);
  return hipGetLastError();
}

hipError_t launch_ema_bwd(const EmaSrc& src, bool polar, const cf* g, const cf* init, const float* rho_logit,
                          const float* theta_raw, cf* gx, cf* ginit, float* g_rho, float* g_th, cf* states, float* part,
                          hipStream_t s) {
  EmaArgs a{};
  a.src = src.ptr; a.tok_stride = src.row_stride; a.init = init; a.rho_logit = rho_logit; a.theta_raw = theta_raw;
  a.g = g; a.gx = gx; a.ginit = ginit; a.states = states; a.part = (g_rho || g_th) ? part : nullptr;
  a.B = src.B; a.S = src.S; a.F = src.F; a.L = src.L;
  if (src.kind == 0) ema_launch<0>(true, polar, a, s);
  else if (src.kind == 1) ema_launch<1>(true, polar, a, s);
  else ema_launch<2>(true, polar, a, s);
  if (g_rho || g_th)
    hipLaunchKernelGGL(k_ema_param_sum, dim3((src.F + EMA_BLOCK - 1) / EMA_BLOCK), dim3(EMA_BLOCK), 0, s, part, g_rho,
                       g_th, src.B, src.F);
  return hipGetLastError();
}

// ---- word-structure targets of byte tokens -------------------------------------------------------------------------------
// Both target functions of the bicameral trainer's heads in one launch (reference fft_lm/phase_clock.py:68-115,
// fft_lm/segmentation_head.py:58-99).  The two delimiter sets differ on purpose: the phase clock breaks words at space
// and the punctuation 33..47, 58..64 only, the boundary label also at brackets, braces and newlines.  A token is
// compared as a number, so an int64 value outside 0..255 is a word byte.
template <typename V> SMX_HD bool is_phase_delim(V v) { return (v >= 32 && v <= 47) || (v >= 58 && v <= 64); }
template <typename V> SMX_HD bool is_boundary_delim(V v) {
  return is_phase_delim(v) || (v >= 91 && v <= 96) || (v >= 123 && v <= 126) || v == 10 || v == 13;
}

// One workgroup per row.  A position needs the start and the end of its word, and a word may span the row:
//   A  bits[w] = the phase-delimiter bits of positions 64 w .. 64 w + 63 (one ballot per wavefront; positions past T
//      count as delimiters, so a word ends at T at the latest);
//   B  thread i owns the words [i WPT, (i + 1) WPT): its highest and lowest delimiter, an inclusive max-scan forward
//      and min-scan backward over the WT_BLOCK summaries, then before[w] = last delimiter in front of word w (-1: none)
//      and after[w] = first delimiter behind it;
//   C  the fill: a position looks at its own 64-bit word first and at before / after only when that has no delimiter on
//      the side in question.
template <int SRC>
__global__ __launch_bounds__(WT_BLOCK) void k_word_targets(const void* __restrict__ tokens, long long row_stride,
                                                           cf* __restrict__ phase, float* __restrict__ boundary, int T) {
  typedef typename EmaTok<SRC>::type TOK;
  constexpr int MAXW = WT_MAX_T / 64, NONE = 0x7fffffff;
  __shared__ unsigned long long bits[MAXW];
  __shared__ int before[MAXW], after[MAXW];
  __shared__ int smax[WT_BLOCK], smin[WT_BLOCK];
  const int tid = threadIdx.x, lane = tid & 63;
  const TOK* row = (const TOK*)tokens + (size_t)blockIdx.x * (size_t)row_stride;
  const size_t o = (size_t)blockIdx.x * (size_t)T;
  if (boundary)
    for (int t = tid; t < T; t += WT_BLOCK) boundary[o + t] = (t == T - 1 || is_boundary_delim(row[t + 1])) ? 1.f : 0.f;
  if (!phase) return;
  const int NW = (T + 63) >> 6;
  for (int base = 0; base < NW * 64; base += WT_BLOCK) {                  // A
    const int p = base + tid;
    const bool d = p >= T || is_phase_delim(row[p]);
    const unsigned long long m = __ballot(d);
    if (lane == 0 && (p >> 6) < NW) bits[p >> 6] = m;
  }
  __syncthreads();
  const int WPT = (NW + WT_BLOCK - 1) / WT_BLOCK;                         // B
  const int w0 = min(tid * WPT, NW), w1 = min(w0 + WPT, NW);
  int hi = -1, lo = NONE;
  for (int w = w0; w < w1; ++w) {
    const unsigned long long m = bits[w];
    if (m) {
      hi = w * 64 + 63 - __builtin_clzll(m);
      if (lo == NONE) lo = w * 64 + __builtin_ctzll(m);
    }
  }
  smax[tid] = hi;
  smin[tid] = lo;
  __syncthreads();
  for (int d = 1; d < WT_BLOCK; d <<= 1) {
    const int a = tid >= d ? smax[tid - d] : -1;
    const int b = tid + d < WT_BLOCK ? smin[tid + d] : NONE;
    __syncthreads();
    smax[tid] = max(smax[tid], a);
    smin[tid] = min(smin[tid], b);
    __syncthreads();
  }
  int run = tid ? smax[tid - 1] : -1;
  for (int w = w0; w < w1; ++w) {
    before[w] = run;
    const unsigned long long m = bits[w];
    if (m) run = w * 64 + 63 - __builtin_clzll(m);
  }
  run = tid + 1 < WT_BLOCK ? smin[tid + 1] : NONE;
  for (int w = w1 - 1; w >= w0; --w) {
    after[w] = run;
    const unsigned long long m = bits[w];
    if (m) run = w * 64 + __builtin_ctzll(m);
  }
  __syncthreads();
  for (int t = tid; t < T; t += WT_BLOCK) {                               // C
    const int w = t >> 6, bit = t & 63;
    const unsigned long long m = bits[w];
    cf out = mk(0.f, 0.f);
    if (!((m >> bit) & 1ull)) {
      const unsigned long long below = m & ((1ull << bit) - 1ull);
      const unsigned long long above = bit == 63 ? 0ull : m & (~0ull << (bit + 1));
      const int last = below ? w * 64 + 63 - __builtin_clzll(below) : before[w];
      const int next = min(above ? w * 64 + __builtin_ctzll(above) : after[w], T);
      const int s = last + 1, n = next - s, q = t - s;
      float sn = 0.f, cs = 1.f;
      if (n > 1) sincospif((float)q / (float)(n - 1), &sn, &cs);          // q == 0: exactly (1, 0)
      out = mk(cs, sn);
    }
    phase[o + t] = out;
  }
}

hipError_t launch_word_targets(const void* tokens, int kind, long long row_stride, float* phase, float* boundary, int B,
                               int T, hipStream_t s) {
  if (kind == 1)
    hipLaunchKernelGGL(k_word_targets<1>, dim3(B), dim3(WT_BLOCK), 0, s, tokens, row_stride, (cf*)phase, boundary, T);
  else
    hipLaunchKernelGGL(k_word_targets<2>, dim3(B), dim3(WT_BLOCK), 0, s, tokens, row_stride, (cf*)phase, boundary, T);
  return hipGetLastError();
}

}  // namespace smx
