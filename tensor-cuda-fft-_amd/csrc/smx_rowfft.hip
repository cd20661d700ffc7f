// smx_rowfft.hip -- the DFT along the contiguous last axis of dense rows (include/smx_rowfft.h states the definition).
// The sequence transform takes its vector width from the channel axis (a lane owns channel pairs); rows of the last axis
// have none, and handing them over as (rows, n, 1) leaves almost every lane idle.  Here a workgroup of 256 threads owns a
// TILE of 4096 consecutive points -- one row of 4096, two of 2048, ... 2048 rows of 2 -- whatever n is, so no wavefront
// idles on short rows; the data is read once and written once.
//
//   load    the tile's points, 16 bytes per lane and access (two complex64 or four fp32), into the LDS image; CONJ_IN here
//   passes  Stockham auto-sort, radices from {16, 8, 4, 2} (pass_bits: log2 n spread evenly over ceil(log2 n / 4) passes:
//           4096 = 16 16 16, 2048 = 16 16 8, 1024 = 16 8 8, 512 = 8 8 8, 32 = 8 4).  In every pass a thread holds 16 points
//           in registers as 16 / R butterflies of radix R (fft16 / fft8 / radix4 of smx_core.h).  Pass p with
//           Ns = the product of the radices before it: butterfly j of a row (j < n / R), k = j mod Ns, reads
//           x[j + q n / R], q < R, multiplies by w^{q k}, w = exp(-2 pi i / (Ns R)), transforms, and writes
//           y[(j div Ns) Ns R + k + q Ns]; after the last pass the image holds the spectrum in natural order.
//           w^k is sincospif of k / (Ns R / 2), an exact binary fraction, and its powers come from powers16 (depth <= 4).
//           All threads read, barrier, all threads write, barrier: the image is transformed in place.
//   store   the image, 16 bytes per lane and access, scaled; CONJ_OUT and REAL_OUT here
// The image is padded by one point after every 16 (PAD): the first pass of a radix-16 plan writes 16 consecutive points
// per lane, 128 bytes apart from lane to lane, which unpadded falls on two bank pairs; padded, lane l's point q is at
// 17 l + q and a half wavefront's 8-byte accesses cover all 64 banks once.  Reads are contiguous over the lanes in every
// pass.  (A point is moved to and from the image as 8 bytes: the pad breaks 16-byte alignment of a pair.)
// Later passes (Ns > 1) write, for a fixed q, runs of min(Ns, 64) consecutive points over the lanes; run g starts
// Ns R points after run g - 1.  By the same arithmetic, not by a counter: Ns = 16 (second pass of 16 16 .) puts the two
// runs of a half wavefront 272 padded points apart, 16 bank pairs, no conflict; Ns >= 64 is one contiguous run; Ns = 8
// (second pass of 8 8 and 8 8 8) puts four runs of 8 at steps of 68 points, 4 bank pairs, so neighbouring runs overlap:
// two-way.  The pad was chosen for the first pass; LDS conflict counters of the later passes have not been read.
//
// A workgroup walks tiles g, g + G, ...; rows is a long long and the grid never exceeds what stays resident.  Only vector
// stores and plain C++; no atomics on memory, no flag words, no workgroup waits for another.  The arithmetic of a row
// depends on its place in the tile only through addresses, never through values: a row's result is a pure function of
// the row, n, flags and scale.  A workgroup has read its tile whole (the barrier after the load) before it stores any of
// it, so out == in is safe when both sides have the same element type.
//
// The launcher at the end of this file is declared in smx_kernels.h (weak there); the C entry is in smx_api.hip.
#include <cstdint>

#include "../../include/smx_rowfft.h"
#include "smx_kernels.h"

namespace smx {

constexpr int ROWFFT_BLOCK = 256;
constexpr int ROWFFT_LOG_TILE = 12, ROWFFT_TILE = 1 << ROWFFT_LOG_TILE;   // points per workgroup and round: 16 per thread
constexpr int ROWFFT_MAX_WG = 4 * 256;                                    // 4 workgroups' images fit a CU's LDS; 256 CUs
static_assert(ROWFFT_TILE == SMX_ROWFFT_MAX_N && ROWFFT_TILE == 16 * ROWFFT_BLOCK, "a tile is one longest row");

struct RowfftArgs {
  const void* in;
  void* out;
  long long rows, tiles;
  int flags;
  float scale;
};

__host__ __device__ constexpr int rowfft_pad(int i) { return i + (i >> 4); }
constexpr int ROWFFT_IMAGE = ROWFFT_TILE + (ROWFFT_TILE >> 4);            // rowfft_pad(TILE - 1) + 1 <= this

// log2 of the radix of pass p of a 2^logn-point row: logn spread over ceil(logn / 4) passes, the larger radices first
__host__ __device__ constexpr int rowfft_pass_bits(int logn, int p) {
  const int np = (logn + 3) / 4;
  return logn / np + (p < logn % np ? 1 : 0);
}

template <int R>
__device__ __forceinline__ void rowfft_bfly(cf (&v)[R]) {
  if constexpr (R == 16) fft16<-1>(v);
  else if constexpr (R == 8) fft8<-1>(v);
  else if constexpr (R == 4) radix4<-1>(v[0], v[1], v[2], v[3]);
  else { const cf a = v[0], b = v[1]; v[0] = cadd(a, b); v[1] = csub(a, b); }
}

// One pass over the image: `nbf` butterflies of radix R are live in this tile (rows_t * n / R), thread t owns butterflies
// t, t + 256, ...: 16 / R of them, 16 points.
template <int LOGN, int LOGR, int LOGNS>
__device__ __forceinline__ void rowfft_pass(cf* img, int nbf) {
  constexpr int R = 1 << LOGR, NB = 16 / R, LOGQ = LOGN - LOGR, Q = 1 << LOGQ, NS = 1 << LOGNS;
  const int tid = threadIdx.x;
  cf v[NB][R];
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int b = tid + u * ROWFFT_BLOCK;
    if (b < nbf) {
      const int at = ((b >> LOGQ) << LOGN) + (b & (Q - 1));
#pragma unroll
      for (int q = 0; q < R; ++q) v[u][q] = img[rowfft_pad(at + q * Q)];
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int b = tid + u * ROWFFT_BLOCK;
    if (b < nbf) {
      const int j = b & (Q - 1), k = j & (NS - 1);
      if constexpr (LOGNS > 0) {
        float sn, cs;
        sincospif((float)k * (-2.f / (float)(NS * R)), &sn, &cs);         // exact argument: k / 2^m
        cf cp[16];
        powers16(mk(cs, sn), cp);
#pragma unroll
        for (int q = 1; q < R; ++q) v[u][q] = cmul(v[u][q], cp[q]);
      }
      rowfft_bfly<R>(v[u]);
      const int at = ((b >> LOGQ) << LOGN) + ((j >> LOGNS) << (LOGNS + LOGR)) + k;
#pragma unroll
      for (int q = 0; q < R; ++q) img[rowfft_pad(at + q * NS)] = v[u][q];
    }
  }
  __syncthreads();
}

template <int LOGN, int P, int LOGNS>
__device__ __forceinline__ void rowfft_passes(cf* img, int rows_t) {
  if constexpr (LOGNS < LOGN) {
    constexpr int LOGR = rowfft_pass_bits(LOGN, P);
    rowfft_pass<LOGN, LOGR, LOGNS>(img, rows_t << (LOGN - LOGR));
    rowfft_passes<LOGN, P + 1, LOGNS + LOGR>(img, rows_t);
  }
}

template <int LOGN>
__global__ __launch_bounds__(ROWFFT_BLOCK) void k_rowfft(RowfftArgs a) {
  constexpr int RPT = ROWFFT_TILE >> LOGN;                                // rows per tile
  __shared__ cf img[ROWFFT_IMAGE];
  const int tid = threadIdx.x;
  const bool conj_in = a.flags & SMX_ROWFFT_CONJ_IN, conj_out = a.flags & SMX_ROWFFT_CONJ_OUT;
  const bool real_in = a.flags & SMX_ROWFFT_REAL_IN, real_out = a.flags & SMX_ROWFFT_REAL_OUT;
  const float scale = a.scale;
  for (long long t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    const long long left = a.rows - t * RPT;
    const int rows_t = left < RPT ? (int)left : RPT;
    const int cnt = rows_t << LOGN;                                       // live points of this tile; even
    const long long e0 = t << ROWFFT_LOG_TILE;                            // its first point
    // ---- load: 16 bytes per lane
    if (real_in) {
      const float* p = static_cast<const float*>(a.in) + e0;
      for (int i = 4 * tid; i < cnt; i += 4 * ROWFFT_BLOCK) {
        if (i + 3 < cnt) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(p + i);
          const float x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int m = 0; m < 4; ++m) { cf c = mk(x[m], 0.f); if (conj_in) c.y = -c.y; img[rowfft_pad(i + m)] = c; }
        } else {                                                          // n == 2, an odd row count: the last two points
          for (int m = i; m < cnt; ++m) { cf c = mk(p[m], 0.f); if (conj_in) c.y = -c.y; img[rowfft_pad(m)] = c; }
        }
      }
    } else {
      const float* p = static_cast<const float*>(a.in) + 2 * e0;
      for (int i = 2 * tid; i < cnt; i += 2 * ROWFFT_BLOCK) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(p + 2 * i);
        cf c0 = mk(w.x, w.y), c1 = mk(w.z, w.w);
        if (conj_in) { c0.y = -c0.y; c1.y = -c1.y; }
        img[rowfft_pad(i)] = c0;
        img[rowfft_pad(i + 1)] = c1;
      }
    }
    __syncthreads();
    // ---- the passes; afterwards the image holds the spectra in natural order
    rowfft_passes<LOGN, 0, 0>(img, rows_t);
    // ---- store: 16 bytes per lane
    if (real_out) {
      float* p = static_cast<float*>(a.out) + e0;
      for (int i = 4 * tid; i < cnt; i += 4 * ROWFFT_BLOCK) {
        if (i + 3 < cnt) {
          f32x4 w;
          w.x = img[rowfft_pad(i)].x * scale; w.y = img[rowfft_pad(i + 1)].x * scale;
          w.z = img[rowfft_pad(i + 2)].x * scale; w.w = img[rowfft_pad(i + 3)].x * scale;
          *reinterpret_cast<f32x4*>(p + i) = w;
        } else {
          for (int m = i; m < cnt; ++m) p[m] = img[rowfft_pad(m)].x * scale;
        }
      }
    } else {
      float* p = static_cast<float*>(a.out) + 2 * e0;
      for (int i = 2 * tid; i < cnt; i += 2 * ROWFFT_BLOCK) {
        const cf c0 = img[rowfft_pad(i)], c1 = img[rowfft_pad(i + 1)];
        f32x4 w;
        w.x = c0.x * scale; w.y = c0.y * scale; w.z = c1.x * scale; w.w = c1.y * scale;
        if (conj_out) { w.y = -w.y; w.w = -w.w; }
        *reinterpret_cast<f32x4*>(p + 2 * i) = w;
      }
    }
    __syncthreads();                                                      // the next tile's load overwrites the image
  }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------------
// rows > 0, rowfft_supported(n), pointers 16-byte aligned, flags within the four bits
hipError_t launch_rowfft(const void* in, void* out, long long rows, int n, int flags, float scale, int max_workgroups,
                         hipStream_t s) {
  int logn = 0;
  while ((1 << logn) < n) ++logn;
  const long long rpt = ROWFFT_TILE >> logn;
  RowfftArgs a{};
  a.in = in; a.out = out; a.rows = rows; a.tiles = (rows + rpt - 1) / rpt; a.flags = flags; a.scale = scale;
  const dim3 grid((unsigned)tile_workgroups(a.tiles, ROWFFT_MAX_WG, max_workgroups)), block(ROWFFT_BLOCK);
  switch (logn) {
#define SMX_ROWFFT_CASE(L) case L: hipLaunchKernelGGL(k_rowfft<L>, grid, block, 0, s, a); break;
    SMX_ROWFFT_CASE(1) SMX_ROWFFT_CASE(2) SMX_ROWFFT_CASE(3) SMX_ROWFFT_CASE(4) SMX_ROWFFT_CASE(5) SMX_ROWFFT_CASE(6)
    SMX_ROWFFT_CASE(7) SMX_ROWFFT_CASE(8) SMX_ROWFFT_CASE(9) SMX_ROWFFT_CASE(10) SMX_ROWFFT_CASE(11) SMX_ROWFFT_CASE(12)
#undef SMX_ROWFFT_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace smx
