// smx_byte.hip -- the byte-spectral feature rows of fft_tensor's byte language model (reference
// fft_tensor/byte_spectral_model.py:44-102, ByteSpectralEmbedding.forward, and fft_tensor/byte_spectral.py:53-108,
// ByteSpectralEncoder.forward) as ONE launch, and the gradient of their band weights as two plain launches.
//
// The reference walks the T positions of a row in Python: roll, a full FFT, abs, angle, a multiply, sin, cos, cat, pad
// per position, about ten launches each.  With s[t] = id[t] / 127.5 - 1 = (2 id[t] - 255) / 255 and
// S[f] = sum_t s[t] e^{-2 pi i f t / T}, the spectrum of roll(s, -pos) is S[f] e^{+2 pi i (f pos mod T) / T} (shift
// theorem), so with u = S / |S| (a zero bin: angle(0) = 0, i.e. sin 0 and cos 1 at EVERY position) column j of the
// feature row at (b, pos) is
//     0 <= j <  k    |S[b, j]| bands[j]
//     k <= j < 2k    Im(u[b, j - k]  tw[(j - k)  pos mod T])
//    2k <= j < 3k    Re(u[b, j - 2k] tw[(j - 2k) pos mod T])            tw[n] = e^{2 pi i n / T}
//    3k <= j         0
// cut at W columns.  The whole (B, P, W) tensor is a function of B k complex numbers: the launch is bound by its store.
//
// One workgroup writes a chunk of `pp` positions of one batch row, and recomputes that row's k bins itself from the row's
// bytes staged in LDS (k T <= 128 x 512 complex multiply-adds at the default shape: less than the store of its chunk)
// instead of a second launch and a (B, k) round trip through memory:
//   A  tw[n], n < T, in LDS by sincospi in double (exact at the quarter turns); the row as the INTEGERS 2 id - 255;
//   B  bin f as a direct sum over tw[f t mod T] -- the index is the exact integer, stepped by f and wrapped, never an
//      accumulated angle -- by NS = 2^n lanes of one wavefront, each over a contiguous slice of t with four interleaved
//      accumulators, joined by a butterfly of lane exchanges (fixed order).  For f > 0 the row's mean, rounded to an integer, is taken
//      off every term: that changes nothing (the twiddles of a bin f > 0 sum to zero), keeps the slices' partial sums from
//      carrying mean x (a slice of a slow twiddle) only to cancel it between slices, and makes a constant row an exact zero;
//   C  u[f] and |S[f]| bands[f] in LDS (u over the row's bytes, which are dead by then: 2k <= T floats);
//   D  the store: a thread keeps its columns and walks the positions of the chunk, the twiddle index of a phase column
//      stepped by (f rows-per-step mod T) and wrapped; whole rows go out as 16-byte vectors (W % 4 == 0).
//
// grad_bands[f] = sum_b sum_p g[b, p, f] |S[b, f]|: per (batch row, 64 positions) partial sums, one lane per column, then
// a sum over the partials in index order by a second launch.  No atomics, no flags: bitwise reproducible.
//
// The launchers and size rules at the end of this file are declared in smx_kernels.h; the C entries are in smx_api.hip.
#include <cstdint>

#include "smx_kernels.h"

namespace smx {

constexpr int BYTE_BLOCK = 256;
constexpr int BYTE_MAX_T = 4096, BYTE_MAX_K = 2048, BYTE_MAX_W = 4096;
constexpr int BYTE_SMALL_T = 512;                       // the instance with 7 KiB of LDS instead of 56
constexpr int BYTE_MAX_PASS = BYTE_MAX_K / BYTE_BLOCK;  // bins one thread can own
constexpr int BYTE_WG_TARGET = 512;                     // workgroups of a launch before rows are cut into fewer chunks
constexpr int BYTE_GB_ROWS = 64;                        // positions per partial sum of the band gradient

// |z| and z / |z| through an exact power-of-two scaling (no overflow or flush of x^2 + y^2); z == 0 -> r = 0, u = (0, 0),
// which step D reads as "no rotation: sin 0, cos 1".
SMX_HD void byte_polar(cf z, float* r, cf* u) {
  const float s = fmaxf(fabsf(z.x), fabsf(z.y));
  if (!(s > 0.f) || !(s < __builtin_inff())) { *r = s > 0.f ? s : 0.f; *u = mk(0.f, 0.f); return; }
  int e;
  (void)frexpf(s, &e);
  const float xs = ldexpf(z.x, -e), ys = ldexpf(z.y, -e);
  const float rs = sqrtf(xs * xs + ys * ys), inv = 1.f / rs;
  *r = ldexpf(rs, e);
  *u = mk(xs * inv, ys * inv);
}

template <typename TOK, bool VEC, int MT>
__global__ __launch_bounds__(BYTE_BLOCK) void k_byte_features(ByteArgs a) {
  __shared__ __align__(16) cf tw[MT];
  __shared__ __align__(16) float sig[MT];                // step C on: u[k] complex
  __shared__ float magb[MT / 2];
  __shared__ float red[BYTE_BLOCK / 64];
  const int tid = threadIdx.x, T = a.T, k = a.k, W = a.W;
  const int b = (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);

  // A
  for (int n = tid; n < T; n += BYTE_BLOCK) {
    double s, c;
    sincospi((double)(2 * n) / (double)T, &s, &c);
    tw[n] = mk((float)c, (float)s);
  }
  const TOK* row = (const TOK*)a.tokens + (size_t)b * (size_t)a.row_stride;
  float mine = 0.f;
  for (int t = tid; t < T; t += BYTE_BLOCK) {
    const float v = fmaf(2.f, (float)row[t], -255.f);
    sig[t] = v;
    mine += v;                                           // bytes: integers below 2^24, exact in any order
  }
  for (int d = 1; d < 64; d <<= 1) mine += __shfl_xor(mine, d);
  if ((tid & 63) == 0) red[tid >> 6] = mine;
  __syncthreads();
  const float mean = rintf(((red[0] + red[1]) + (red[2] + red[3])) / (float)T);

  // B
  const int NS = 1 << a.ns_log, bpp = BYTE_BLOCK >> a.ns_log;
  const int sl = tid & (NS - 1), fl = tid >> a.ns_log;
  const int len = (T + NS - 1) >> a.ns_log;
  const int t0 = min(sl * len, T), t1 = min(t0 + len, T);
  cf S[BYTE_MAX_PASS];
#pragma unroll
  for (int p = 0; p < BYTE_MAX_PASS; ++p) {
    S[p] = mk(0.f, 0.f);
    if (p * bpp < k) {                                   // the same for every thread of the workgroup
      const int f = p * bpp + fl;
      float re = 0.f, im = 0.f;
      if (f < k) {
        const float base = f ? mean : 0.f;
        int idx = (int)(((unsigned)f * (unsigned)t0) % (unsigned)T);
        float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f, i0 = 0.f, i1 = 0.f, i2 = 0.f, i3 = 0.f;
        int t = t0;
#define BYTE_TERM(R, I, TT)                          \
  {                                                  \
    const float d = sig[TT] - base;                  \
    const cf w = tw[idx];                            \
    R = fmaf(d, w.x, R);                             \
    I = fmaf(d, w.y, I);                             \
    idx += f;                                        \
    if (idx >= T) idx -= T;                          \
  }
        for (; t + 4 <= t1; t += 4) {
          BYTE_TERM(r0, i0, t)
          BYTE_TERM(r1, i1, t + 1)
          BYTE_TERM(r2, i2, t + 2)
          BYTE_TERM(r3, i3, t + 3)
        }
        for (; t < t1; ++t) BYTE_TERM(r0, i0, t)
#undef BYTE_TERM
        re = (r0 + r1) + (r2 + r3);
        im = -((i0 + i1) + (i2 + i3));                   // e^{-i phi}
      }
      for (int d = 1; d < NS; d <<= 1) {                 // the NS lanes of a bin are neighbours in one wavefront
        re += __shfl_xor(re, d);
        im += __shfl_xor(im, d);
      }
      S[p] = mk(re, im);
    }
  }
  __syncthreads();                                       // the row's bytes are dead

  // C
  cf* un = reinterpret_cast<cf*>(sig);
#pragma unroll
  for (int p = 0; p < BYTE_MAX_PASS; ++p) {
    const int f = p * bpp + fl;
    if (sl == 0 && f < k) {
      float r;
      cf u;
      byte_polar(mk(S[p].x / 255.f, S[p].y / 255.f), &r, &u);
      un[f] = u;
      magb[f] = r * a.bands[f];
      if (a.mag && chunk == 0) a.mag[(size_t)b * k + f] = r;
    }
  }
  __syncthreads();

  // D
  constexpr int V = VEC ? 4 : 1;
  const int npos = a.P == 1 ? 1 : T;
  const int pos0 = chunk * a.pp, pos1 = min(pos0 + a.pp, npos);
  const int CW = 1 << a.cw_log, RY = BYTE_BLOCK >> a.cw_log;
  const int cx = tid & (CW - 1), ry = tid >> a.cw_log;
  const int NC = VEC ? W >> 2 : W;
  float* orow = a.out + (size_t)b * (size_t)a.P * (size_t)W;
  for (int c = cx; c < NC; c += CW) {
    float val[V];                                        // kind 0: the column's value at every position
    cf u[V];
    int kind[V], idx[V], step[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int j = c * V + v;
      kind[v] = 0; val[v] = 0.f; u[v] = mk(0.f, 0.f); idx[v] = 0; step[v] = 0;
      if (j < k) val[v] = magb[j];
      else if (j < 3 * k) {
        const bool is_cos = j >= 2 * k;
        const int f = is_cos ? j - 2 * k : j - k;
        u[v] = un[f];
        if (u[v].x == 0.f && u[v].y == 0.f) val[v] = is_cos ? 1.f : 0.f;
        else {
          kind[v] = is_cos ? 2 : 1;
          idx[v] = (int)(((unsigned)f * (unsigned)(pos0 + ry)) % (unsigned)T);
          step[v] = (int)(((unsigned)f * (unsigned)RY) % (unsigned)T);
        }
      }
    }
    for (int p = pos0 + ry; p < pos1; p += RY) {
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (kind[v] == 0) o[v] = val[v];
        else {
          const cf w = tw[idx[v]];
          o[v] = kind[v] == 1 ? fmaf(u[v].x, w.y, u[v].y * w.x) : fmaf(u[v].x, w.x, -(u[v].y * w.y));
          idx[v] += step[v];
          if (idx[v] >= T) idx[v] -= T;
        }
      }
      float* q = orow + (size_t)p * (size_t)W + (size_t)c * V;
      if constexpr (VEC) *reinterpret_cast<float4*>(q) = make_float4(o[0], o[1], o[2], o[3]);
      else *q = o[0];
    }
  }
}

// part[chunk, f] = mag[b, f] sum_{p in chunk} g[b, p, f], p ascending in four interleaved sums; chunk = b CP + cp
__global__ __launch_bounds__(64) void k_byte_gb_part(const float* __restrict__ g, const float* __restrict__ mag,
                                                     float* __restrict__ part, int P, int W, int k, int kk, int CP,
                                                     int tiles) {
  const int chunk = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
  const int f = tile * 64 + threadIdx.x;
  if (f >= kk) return;
  const int b = chunk / CP, p0 = (chunk % CP) * BYTE_GB_ROWS, p1 = min(p0 + BYTE_GB_ROWS, P);
  const float* gp = g + ((size_t)b * (size_t)P) * (size_t)W + f;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int p = p0;
  for (; p + 4 <= p1; p += 4) {
    s0 += gp[(size_t)p * W];
    s1 += gp[(size_t)(p + 1) * W];
    s2 += gp[(size_t)(p + 2) * W];
    s3 += gp[(size_t)(p + 3) * W];
  }
  for (; p < p1; ++p) s0 += gp[(size_t)p * W];
  part[(size_t)chunk * kk + f] = ((s0 + s1) + (s2 + s3)) * mag[(size_t)b * k + f];
}

// grad[f] = sum_chunk part[chunk, f], chunk ascending in four interleaved sums (f < kk); 0 for kk <= f < n
__global__ __launch_bounds__(BYTE_BLOCK) void k_byte_gb_sum(const float* __restrict__ part, float* __restrict__ grad,
                                                            int nchunk, int kk, int n) {
  const int f = blockIdx.x * BYTE_BLOCK + threadIdx.x;
  if (f >= n) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (f < kk) {
    int c = 0;
    for (; c + 4 <= nchunk; c += 4) {
      s0 += part[(size_t)c * kk + f];
      s1 += part[(size_t)(c + 1) * kk + f];
      s2 += part[(size_t)(c + 2) * kk + f];
      s3 += part[(size_t)(c + 3) * kk + f];
    }
    for (; c < nchunk; ++c) s0 += part[(size_t)c * kk + f];
  }
  grad[f] = (s0 + s1) + (s2 + s3);
}

namespace {

int pow2_floor_log(int v) { int l = 0; while ((2 << l) <= v) ++l; return l; }
int pow2_ceil_log(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

template <typename TOK, bool VEC>
void byte_launch_t(const ByteArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((long long)a.B * a.chunks)), block(BYTE_BLOCK);
  if (a.T <= BYTE_SMALL_T) hipLaunchKernelGGL((k_byte_features<TOK, VEC, BYTE_SMALL_T>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_byte_features<TOK, VEC, BYTE_MAX_T>), grid, block, 0, s, a);
}

int gb_chunks_per_row(int P) { return (P + BYTE_GB_ROWS - 1) / BYTE_GB_ROWS; }

}  // namespace

bool byte_supported(int T, int k, int W) {
  return T >= 1 && T <= BYTE_MAX_T && k >= 0 && k <= T / 2 && k <= BYTE_MAX_K && W >= 1 && W <= BYTE_MAX_W;
}

hipError_t launch_byte_features(const void* tokens, int kind, long long row_stride, const float* bands, float* out,
                                float* mag, int B, int T, int k, int W, int P, hipStream_t s) {
  ByteArgs a{};
  a.tokens = tokens; a.row_stride = row_stride; a.bands = bands; a.out = out; a.mag = mag;
  a.B = B; a.T = T; a.k = k; a.W = W; a.P = P;
  const int npos = a.P == 1 ? 1 : a.T;
  // Every workgroup recomputes its row's bins, so a row is cut into few chunks once the batch alone fills the chip
  // (about 512 workgroups, two per CU): at least 16 positions each, at most 32 chunks of a long row.
  const int want = BYTE_WG_TARGET / a.B > 0 ? BYTE_WG_TARGET / a.B : 1;
  a.pp = (npos + want - 1) / want;
  if (a.pp < 16) a.pp = 16;
  if (a.T > BYTE_SMALL_T && a.pp < (a.T + 31) / 32) a.pp = (a.T + 31) / 32;
  if (a.pp > npos) a.pp = npos;
  a.chunks = (npos + a.pp - 1) / a.pp;
  a.ns_log = a.k > 0 ? pow2_floor_log(BYTE_BLOCK / (a.k < BYTE_BLOCK ? a.k : BYTE_BLOCK)) : 0;
  if (a.ns_log > 6) a.ns_log = 6;
  const bool vec = a.W % 4 == 0;
  a.cw_log = pow2_ceil_log(vec ? a.W / 4 : a.W);
  if (a.cw_log > 8) a.cw_log = 8;
  if (kind == 1) {
    if (vec) byte_launch_t<unsigned char, true>(a, s);
    else byte_launch_t<unsigned char, false>(a, s);
  } else {
    if (vec) byte_launch_t<long long, true>(a, s);
    else byte_launch_t<long long, false>(a, s);
  }
  return hipGetLastError();
}

long long byte_gb_blocks(int B, int P, int kk) {
  const int tiles = (kk + 63) / 64;
  return (long long)B * gb_chunks_per_row(P) * (tiles > 0 ? tiles : 1);
}
size_t byte_gb_part_bytes(int B, int P, int kk) { return al((size_t)B * gb_chunks_per_row(P) * kk * sizeof(float)); }

hipError_t launch_byte_grad_bands(const float* g, const float* mag, float* part, float* grad_bands, int n_bands, int B,
                                  int P, int W, int k, hipStream_t s) {
  const int kk = k < W ? k : W, CP = gb_chunks_per_row(P);
  const int nchunk = B * CP, tiles = (kk + 63) / 64;
  if (kk > 0)
    hipLaunchKernelGGL(k_byte_gb_part, dim3((unsigned)((long long)nchunk * tiles)), dim3(64), 0, s, g, mag, part, P, W, k,
                       kk, CP, tiles);
  hipLaunchKernelGGL(k_byte_gb_sum, dim3((unsigned)((n_bands + BYTE_BLOCK - 1) / BYTE_BLOCK)), dim3(BYTE_BLOCK), 0, s,
                     (const float*)part, grad_bands, nchunk, kk, n_bands);
  return hipGetLastError();
}

}  // namespace smx
