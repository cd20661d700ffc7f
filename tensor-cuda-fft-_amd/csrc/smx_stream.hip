// smx_stream.hip -- overlap-save chunk generation: one chunk step of a FixedSpectralBlock at inference
// (reference scripts/generate_chunked_overlap_save.py:101-172) as two row-kernel launches around the block's
// gate_ctx GEMV.
//
// The reference, per layer and per emitted chunk, normalises the chunk, torch.cat's the whole (1, T, C) window, sums
// it, transforms K - 1 + chunk rows zero-padded to n_fft points forth and back and keeps `chunk` of the n_fft output
// rows.  At inference the filter spectrum H = k_freq sigmoid(gate_freq) (x cutoff mask) is a constant and so is its
// inverse transform h_eff (n_fft real taps, NOT compact: the gate smears the K-tap kernel over the whole period).  The
// reference's product of spectra is the circular convolution y_pad[m] = sum_j h_eff[(m - j) mod n_fft] x_seg[j] with
// x_seg zero beyond L = K - 1 + chunk rows, and the kept rows are m = K - 1 + n, n < chunk:
//     y[n] = sum_{j < L} taps[n + L - 1 - j] seg[j],      taps[i] = h_eff[(i - (chunk - 1)) mod n_fft]
// -- lags m - j from -(chunk - 1) (the wrap the reference's FFT includes) to K + chunk - 2: K + 2 chunk - 2 taps.
//
//   k_stream_push   the window of LayerNorm outputs is a ring (Bt, T, C) that is never copied; pos[b] (device memory,
//                   so that a captured graph follows the ring) is the slot of the oldest row.  One workgroup per batch
//                   row -- the only reader and writer of that row's pos -- normalises the chunk's rows, one wavefront
//                   per row, swaps them for the evicted ones and keeps the window sum as a compensated pair (hi, lo):
//                   the reference re-sums the window every chunk, an incremental fp32 sum would drift over thousands
//                   of chunks, a two-sum costs two more flops per element.
//   k_stream_conv   a workgroup owns R output rows of one batch row; its ROW_WAVES wavefronts split the j range
//                   (j = wave, wave + ROW_WAVES, ...), each loaded ring row feeds R taps, the partial rows are added in
//                   wavefront order through LDS, and wavefront r finishes row r: residual, scale = gain g_ctx, and the
//                   FFN's LayerNorm.  The sums do not depend on R or on the batch size: bitwise reproducible.
// One wavefront per row, lane l holding elements (l + 64 c) VEC + [0, VEC), c < CH (smx_rows.h).
#include "smx_kernels.h"
#include "smx_rows.h"

namespace smx {

namespace {

constexpr int STREAM_MAX_TAPS = STREAM_MAX_K + 2 * STREAM_MAX_CHUNK - 2;

// pos as the kernels use it: in [0, T) whatever the word holds, so that no slot can leave the ring
__device__ __forceinline__ int ring_pos(const int* pos, int b, int T) {
  const int p = pos[b] % T;
  return p < 0 ? p + T : p;
}

// r = (r - mean) rstd gamma + beta on the C valid elements, 0 on the padding
template <int VEC, int CH>
__device__ __forceinline__ void row_norm(Vec<VEC> (&r)[CH], const float* ln_w, const float* ln_b, float eps, int C,
                                         int lane) {
  const cf st = row_stats(r, C, lane, eps);
  Vec<VEC> gm[CH], bt[CH];
  row_load_cached(gm, ln_w, C, lane, 1.f);
  row_load_cached(bt, ln_b, C, lane, 0.f);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const bool in = (lane + 64 * c) * VEC < C;
#pragma unroll
    for (int i = 0; i < VEC; ++i) r[c].v[i] = in ? fmaf((r[c].v[i] - st.x) * st.y, gm[c].v[i], bt[c].v[i]) : 0.f;
  }
}

template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_stream_push(const float* __restrict__ h,
                                                                const float* __restrict__ ln_w,
                                                                const float* __restrict__ ln_b, float eps,
                                                                float* __restrict__ ring, float* __restrict__ sum,
                                                                int* __restrict__ pos, float* __restrict__ pooled, int T,
                                                                int C, int chunk) {
  __shared__ float red[ROW_WAVES][64 * VEC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const int p = ring_pos(pos, b, T);          // (rewritten by thread 0 behind the barriers below)
  float* rb = ring + (size_t)b * T * C;
  Vec<VEC> acc[CH];
  zero(acc);
  for (int n = wv; n < chunk; n += ROW_WAVES) {
    int slot = p + n;                         // chunk <= T
    if (slot >= T) slot -= T;
    float* rr = rb + (size_t)slot * C;
    Vec<VEC> x[CH], ev[CH];
    row_load(x, h + ((size_t)b * chunk + n) * C, C, lane);
    row_load(ev, rr, C, lane);
    row_norm(x, ln_w, ln_b, eps, C, lane);
    row_store(x, rr, C, lane);
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[c].v[i] += x[c].v[i] - ev[c].v[i];
  }
  float* sb = sum + (size_t)b * 2 * C;
  const float inv_t = 1.f / (float)T;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) red[wv][lane * VEC + i] = acc[c].v[i];
    __syncthreads();
    const int e = (lane + 64 * c) * VEC;
    if (wv == 0 && e < C) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float d = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < ROW_WAVES; ++w2) d += red[w2][lane * VEC + i];
        // (hi, lo) += d: two-sum of hi + d, its error into lo, renormalised
        const float hi = sb[e + i], lo = sb[C + e + i];
        const float s = hi + d;
        const float bb = s - hi;
        const float err = (hi - (s - bb)) + (d - bb);
        const float l2 = lo + err;
        const float h2 = s + l2;
        const float l3 = l2 - (h2 - s);
        sb[e + i] = h2;
        sb[C + e + i] = l3;
        pooled[(size_t)b * C + e + i] = (h2 + l3) * inv_t;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int q = p + chunk;
    if (q >= T) q -= T;
    pos[b] = q;
  }
}

template <int VEC, int CH, int R>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_stream_conv(const float* h, const float* __restrict__ ring,
                                                                const int* __restrict__ pos,
                                                                const float* __restrict__ taps,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ ln_w,
                                                                const float* __restrict__ ln_b, float eps, float* h_out,
                                                                float* __restrict__ ff_in, int T, int K, int C,
                                                                int chunk) {
  static_assert(R <= ROW_WAVES, "wavefront r finishes output row r");
  __shared__ float tp[STREAM_MAX_TAPS];
  __shared__ float red[ROW_WAVES][R][64 * VEC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int L = K - 1 + chunk, groups = (chunk + R - 1) / R;
  const int b = blockIdx.x / groups, n0 = (blockIdx.x % groups) * R;
  for (int i = threadIdx.x; i < L + chunk - 1; i += 64 * ROW_WAVES) tp[i] = taps[i];
  __syncthreads();
  int base = ring_pos(pos, b, T) - L;         // L <= T
  if (base < 0) base += T;
  const float* rb = ring + (size_t)b * T * C;
  Vec<VEC> acc[R][CH];
#pragma unroll
  for (int r = 0; r < R; ++r) zero(acc[r]);
  for (int j = wv; j < L; j += ROW_WAVES) {
    int slot = base + j;
    if (slot >= T) slot -= T;
    Vec<VEC> x[CH];                           // through the caches: the other workgroups of this batch row read it too
    row_load_cached(x, rb + (size_t)slot * C, C, lane, 0.f);
    const float* tj = tp + n0 + (L - 1 - j);  // taps[n + L - 1 - j], n = n0 + r
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (n0 + r < chunk) {
        const float t = tj[r];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[r][c].v[i] = fmaf(t, x[c].v[i], acc[r][c].v[i]);
      }
    }
  }
  Vec<VEC> y[CH];
  zero(y);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int i = 0; i < VEC; ++i) red[wv][r][lane * VEC + i] = acc[r][c].v[i];
    __syncthreads();
    if (wv < R) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float d = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < ROW_WAVES; ++w2) d += red[w2][wv][lane * VEC + i];
        y[c].v[i] = d;
      }
    }
    __syncthreads();
  }
  const int n = n0 + wv;
  if (wv >= R || n >= chunk) return;
  const size_t off = ((size_t)b * chunk + n) * C;
  Vec<VEC> hx[CH], sc[CH];
  row_load(hx, h + off, C, lane);
  row_load_cached(sc, scale + (size_t)b * C, C, lane, 0.f);
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < VEC; ++i) hx[c].v[i] = fmaf(sc[c].v[i], y[c].v[i], hx[c].v[i]);
  row_store(hx, h_out + off, C, lane);
  if (ff_in) {
    row_norm(hx, ln_w, ln_b, eps, C, lane);
    row_store(hx, ff_in + off, C, lane);
  }
}

// the widths ln_supported admits: Vec<4> chunks for C % 4 == 0, the scalar variant otherwise
template <typename Fn>
bool stream_dispatch(int C, Fn f) {
  return C % 4 == 0 ? row_dispatch<4, 16>(C, f) : row_dispatch<1, 16, 4>(C, f);
}

constexpr int STREAM_ACC_REGS = 64;      // accumulator registers a lane may hold: R VEC CH <= 64 (no scratch)
constexpr int STREAM_FILL = 256;         // workgroups that fill the chip: below it a workgroup carries fewer rows

}  // namespace

bool stream_supported(int T, int K, int C, int chunk) {
  return ln_supported(C) && chunk >= 1 && chunk <= STREAM_MAX_CHUNK && K >= 1 && K <= STREAM_MAX_K &&
         (long long)K - 1 + chunk <= T;
}

hipError_t launch_stream_push(const float* h, const float* ln_w, const float* ln_b, float eps, float* ring, float* sum,
                              int* pos, float* pooled, int Bt, int T, int C, int chunk, hipStream_t s) {
  if (Bt < 1 || !stream_supported(T, 1, C, chunk)) return hipErrorInvalidValue;
  stream_dispatch(C, [&](auto vec, auto ch) {
    hipLaunchKernelGGL((k_stream_push<decltype(vec)::value, decltype(ch)::value>), dim3(Bt), dim3(64 * ROW_WAVES), 0, s, h,
                       ln_w, ln_b, eps, ring, sum, pos, pooled, T, C, chunk);
  });
  return hipGetLastError();
}

hipError_t launch_stream_conv(const float* h, const float* ring, const int* pos, const float* taps, const float* scale,
                              const float* ln_w, const float* ln_b, float eps, float* h_out, float* ff_in, int Bt, int T,
                              int K, int C, int chunk, hipStream_t s) {
  if (Bt < 1 || !stream_supported(T, K, C, chunk)) return hipErrorInvalidValue;
  stream_dispatch(C, [&](auto vec, auto ch) {
    constexpr int V = decltype(vec)::value, CHN = decltype(ch)::value;
    // Rows per workgroup: each ring row a wavefront loads feeds R taps, so R divides the L2 reads by R and costs
    // R VEC CH accumulator registers; while the grid does not fill the chip the re-reads are free and rows spread out.
    auto go = [&](auto rr) {
      constexpr int R = decltype(rr)::value;
      hipLaunchKernelGGL((k_stream_conv<V, CHN, R>), dim3((unsigned)Bt * ((chunk + R - 1) / R)), dim3(64 * ROW_WAVES), 0,
                         s, h, ring, pos, taps, scale, ln_w, ln_b, eps, h_out, ff_in, T, K, C, chunk);
    };
    auto fits = [&](int R) { return R * V * CHN <= STREAM_ACC_REGS && (long long)Bt * ((chunk + R - 1) / R) >= STREAM_FILL; };
    if (fits(4)) go(std::integral_constant<int, (4 * V * CHN <= STREAM_ACC_REGS ? 4 : 1)>());
    else if (fits(2)) go(std::integral_constant<int, (2 * V * CHN <= STREAM_ACC_REGS ? 2 : 1)>());
    else go(std::integral_constant<int, 1>());
  });
  return hipGetLastError();
}

}  // namespace smx
