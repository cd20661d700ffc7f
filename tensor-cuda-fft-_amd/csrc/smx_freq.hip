// smx_freq.hip -- the two native ops of the frequency-domain transformer (reference fft_tensor/frequency_ops.py):
// FrequencyAttention.frequency_attention (:147-185, nine whole-tensor ops) and frequency_layernorm (:384-401, about ten).
//
// frequency_attention, complex64 q, k, v (B, H, N, D):
//   s[b, h, n] = mean_d |q conj(k)| / temperature = scale sum_d |q_d| |k_d|,   scale = 1 / (temperature D)
//   p = softmax_n(s),   out[b, h, n, :] = p[b, h, n] v[b, h, n, :]
// (|q conj(k)| = |q| |k|: two square roots and a product, no cancellation; it overflows only where |q| |k| does.)
// Two launches, no atomics on memory, no flag words, no workgroup waits for another:
//   k_fattn_scores  one wavefront per (b, h, n) row streams the q and k rows once (16-byte loads of the interleaved row,
//                   any D), sums in a fixed order (wave_sum) and writes one fp32 score into a (B, H, N) workspace.
//   k_fattn_apply   grid = (tiles of n) x (b h).  Every workgroup first reduces max_n s and sum_n exp(s - max) over ALL N
//                   scores of its (b, h) in a fixed order (thread t takes t, t + 256, ...; lanes by shuffles; the four waves
//                   in index order), so every workgroup of a (b, h) holds the same bits; then a wavefront per row writes
//                   p_n v[n, :] for the rows of the tile.
// Every operand has element strides for b, h and n, the innermost axis contiguous: a (B, N, H, hd) tensor is read as its
// (B, H, N, hd) view and the result lands in (B, N, H hd) layout.  A row is 8-byte aligned at least.  With off = 1 where
// it starts 8 bytes past a 16-byte boundary, pair p holds elements 2p - off and 2p - off + 1: a pair wholly inside the row
// is ONE 16-byte access, a pair cut by either end is moved element by element (nothing outside the row is touched).  Two
// rows walked together (q with k, v with out) share the pairs when their offsets agree; otherwise that row goes element by
// element (8-byte accesses).
//
// frequency_layernorm, per complex row z of D:  m = |z|, mean = mean_d m, std = the UNBIASED deviation of m (torch.std),
//   out = (m - mean) / (std + eps) u(z),  u = z / |z|, u = 1 at z == 0  (exp(i angle(0)) = 1).  D = 1: 0 / 0 = NaN.
// One launch, one wavefront per row, the 2 D floats of the row in registers (smx_rows.h: Vec<4> chunks for an even D,
// whose rows are 16-byte aligned, Vec<2> for an odd one), 16 bytes of traffic per element.  |z| is sqrt(re^2 + im^2) in
// fp32: a |z| below ~1e-19 counts as 0, one above ~1e19 as inf.
//
// The launchers at the end of this file are declared in smx_kernels.h; the C entries are in smx_api.hip.
#include <cstdint>

#include "smx_kernels.h"
#include "smx_rows.h"

namespace smx {

namespace {

constexpr int FATTN_BLOCK = 256;
constexpr int FATTN_WAVES = FATTN_BLOCK / 64;
constexpr int FATTN_SROWS = 16;                            // rows of a workgroup of k_fattn_scores: four per wavefront

__device__ __forceinline__ float2 ld_c(const float2* p) {
  const f32x2 w = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p));
  return make_float2(w.x, w.y);
}
__device__ __forceinline__ float4 ld_c2(const float2* p) {
  const f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(w.x, w.y, w.z, w.w);
}
__device__ __forceinline__ int row_off(const void* p) { return (int)(((uintptr_t)p >> 3) & 1); }
__device__ __forceinline__ float cmag2(float ar, float ai, float br, float bi) {
  return sqrtf(fmaf(ar, ar, ai * ai)) * sqrtf(fmaf(br, br, bi * bi));
}

// the row (b, h, n) of an operand with element strides (sb, sh, sn)
__device__ __forceinline__ long long row_at(const long long (&st)[3], long long b, long long h, long long n) {
  return b * st[0] + h * st[1] + n * st[2];
}
// the wavefront of the workgroup, as a scalar: what hangs on it (row numbers, row addresses) is then scalar arithmetic
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// grid = (blocks of FATTN_SROWS rows of n) x (b h): the (b, h) of a workgroup costs one scalar division, a row none
__global__ __launch_bounds__(FATTN_BLOCK) void k_fattn_scores(FattnArgs a, float* __restrict__ scores, int nblk) {
  const int lane = threadIdx.x & 63, wv = wave_id(), D = a.D, N = a.N;
  const unsigned bh = blockIdx.x / (unsigned)nblk, t = blockIdx.x - bh * (unsigned)nblk;
  const unsigned b = bh / (unsigned)a.H, h = bh - b * (unsigned)a.H;
  const int n1 = (int)((t + 1) * FATTN_SROWS) < N ? (int)((t + 1) * FATTN_SROWS) : N;
  for (int n = (int)(t * FATTN_SROWS) + wv; n < n1; n += FATTN_WAVES) {
    const float2* q = a.q + row_at(a.sq, b, h, n);
    const float2* k = a.k + row_at(a.sk, b, h, n);
    const int off = row_off(q);
    float s = 0.f;
    if (off == row_off(k)) {
      const int np = (off + D + 1) >> 1;
      for (int p = lane; p < np; p += 64) {
        const int i0 = 2 * p - off;
        if (i0 >= 0 && i0 + 1 < D) {
          const float4 x = ld_c2(q + i0), y = ld_c2(k + i0);
          s += cmag2(x.x, x.y, y.x, y.y) + cmag2(x.z, x.w, y.z, y.w);
        } else {
          if (i0 >= 0) { const float2 x = ld_c(q + i0), y = ld_c(k + i0); s += cmag2(x.x, x.y, y.x, y.y); }
          if (i0 + 1 < D) { const float2 x = ld_c(q + i0 + 1), y = ld_c(k + i0 + 1); s += cmag2(x.x, x.y, y.x, y.y); }
        }
      }
    } else {
      for (int i = lane; i < D; i += 64) { const float2 x = ld_c(q + i), y = ld_c(k + i); s += cmag2(x.x, x.y, y.x, y.y); }
    }
    s = wave_sum(s);
    if (lane == 0) scores[(long long)bh * N + n] = s * a.scale;
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

__global__ __launch_bounds__(FATTN_BLOCK) void k_fattn_apply(FattnArgs a, const float* __restrict__ scores, int tile_n,
                                                             int tiles) {
  __shared__ float red[2][FATTN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
  const unsigned bh = blockIdx.x / (unsigned)tiles, t = blockIdx.x - bh * (unsigned)tiles;
  const unsigned b = bh / (unsigned)a.H, h = bh - b * (unsigned)a.H;
  const int N = a.N, D = a.D;
  const float* s = scores + (long long)bh * N;
  // the statistics of the whole (b, h): the same instructions on the same values in every workgroup of it
  float mx = -INFINITY;
  for (int i = tid; i < N; i += FATTN_BLOCK) mx = fmaxf(mx, s[i]);
  mx = wave_max(mx);
  if (lane == 0) red[0][wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  float sum = 0.f;
  for (int i = tid; i < N; i += FATTN_BLOCK) sum += expf(s[i] - mx);
  sum = wave_sum(sum);
  if (lane == 0) red[1][wv] = sum;
  __syncthreads();
  sum = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  const int n1 = (int)((t + 1) * tile_n) < N ? (int)((t + 1) * tile_n) : N;
  for (int n = (int)(t * tile_n) + wv; n < n1; n += FATTN_WAVES) {
    const float p = expf(s[n] - mx) / sum;
    const float2* v = a.v + row_at(a.sv, b, h, n);
    float2* o = a.out + row_at(a.so, b, h, n);
    const int off = row_off(v);
    if (off == row_off(o)) {
      const int np = (off + D + 1) >> 1;
      for (int q = lane; q < np; q += 64) {
        const int i0 = 2 * q - off;
        if (i0 >= 0 && i0 + 1 < D) {
          const float4 x = ld_c2(v + i0);
          *reinterpret_cast<float4*>(o + i0) = make_float4(p * x.x, p * x.y, p * x.z, p * x.w);
        } else {
          if (i0 >= 0) { const float2 x = ld_c(v + i0); o[i0] = make_float2(p * x.x, p * x.y); }
          if (i0 + 1 < D) { const float2 x = ld_c(v + i0 + 1); o[i0 + 1] = make_float2(p * x.x, p * x.y); }
        }
      }
    } else {
      for (int i = lane; i < D; i += 64) { const float2 x = ld_c(v + i); o[i] = make_float2(p * x.x, p * x.y); }
    }
  }
}

// One wavefront per row of W = 2 D floats, rows walked ROW_WAVES at a time (row_launch).
template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_freq_ln(const float* __restrict__ z, float* __restrict__ out, float eps,
                                                            long long rows, int D) {
  constexpr int PER = VEC / 2;                             // complex elements of a chunk
  const int lane = threadIdx.x & 63, W = 2 * D;
  const float inv_d = 1.f / (float)D;
  for (long long r = (long long)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * ROW_WAVES) {
    Vec<VEC> x[CH];
    row_load(x, z + r * W, W, lane);                       // zeros past the row: m = 0 there
    float m[CH][PER], s = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        m[c][j] = sqrtf(fmaf(x[c].v[2 * j], x[c].v[2 * j], x[c].v[2 * j + 1] * x[c].v[2 * j + 1]));
        s += m[c][j];
      }
    const float mean = wave_sum(s) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
#pragma unroll
      for (int j = 0; j < PER; ++j)
        if (e + 2 * j < W) { const float d = m[c][j] - mean; sq = fmaf(d, d, sq); }
    }
    const float var = wave_sum(sq) / (float)(D - 1);       // D = 1: 0 / 0
    const float scale = 1.f / (sqrtf(var) + eps);
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const float g = (m[c][j] - mean) * scale;
        const bool nz = m[c][j] > 0.f;
        const float f = g / (nz ? m[c][j] : 1.f);
        x[c].v[2 * j] = nz ? f * x[c].v[2 * j] : g;
        x[c].v[2 * j + 1] = nz ? f * x[c].v[2 * j + 1] : 0.f;
      }
    row_store(x, out + r * W, W, lane);
  }
}

}  // namespace

hipError_t launch_freq_ln(const float* z, float* out, float eps, long long rows, int D, hipStream_t s) {
  auto go = [&](auto vec, auto ch) {
    row_launch(k_freq_ln<decltype(vec)::value, decltype(ch)::value>, rows, s, z, out, eps, rows, D);
  };
  const bool ok = D % 2 == 0 ? row_dispatch<4, 8>(2 * D, go) : row_dispatch<2, 16, 4>(2 * D, go);
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// rows of a tile of k_fattn_apply: 64, doubled while more than FATTN_MAX_WG workgroups would remain (each re-reads the N
// scores of its (b, h) from cache: with more rows per tile that read shrinks against the tile's own traffic)
int fattn_tile_rows(long long BH, int N) {
  int tile = 64;
  while (tile < N && BH * ((N + tile - 1) / tile) > FATTN_MAX_WG) tile *= 2;
  return tile;
}

hipError_t launch_fattn(const FattnArgs& a, float* scores, hipStream_t s) {
  const long long BH = a.rows / a.N;
  const int tile = fattn_tile_rows(BH, a.N), tiles = (a.N + tile - 1) / tile;
  const int nblk = (a.N + FATTN_SROWS - 1) / FATTN_SROWS;
  hipLaunchKernelGGL(k_fattn_scores, dim3((unsigned)(BH * nblk)), dim3(FATTN_BLOCK), 0, s, a, scores, nblk);
  hipLaunchKernelGGL(k_fattn_apply, dim3((unsigned)(BH * tiles)), dim3(FATTN_BLOCK), 0, s, a, (const float*)scores, tile,
                     tiles);
  return hipGetLastError();
}

}  // namespace smx
