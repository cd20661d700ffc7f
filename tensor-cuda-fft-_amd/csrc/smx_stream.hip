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
//
// Also here, as the other launch of a generated chunk: k_sample_bytes, the byte sampler (at the end of the file).
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

// ---- the byte sampler: penalties over a recent window, bans, temperature, nucleus, top-k and the draw, one launch ----
// (reference fft_lm/train_fixed_full.py:651-701, scripts/stream_generate_fast.py:146-170,
// scripts/generate_chunked_overlap_save.py:39-48, 283-292: all one function of a 256-wide row, include/smx.h.)
// One workgroup of SAMPLE_V threads per row, thread t owns logit t.  Every sum over the row is a block scan in a fixed
// order -- a shuffle scan inside each wavefront, the wavefront totals added in wavefront order -- so a row's result
// does not depend on the other rows of the call or on the run: bitwise reproducible.  The window counts are integer LDS
// additions (exact in any order).  Nothing in global memory is written but ids[r] and probs[r, :].
namespace {

constexpr int SAMPLE_WAVES = SAMPLE_V / 64;

struct SampleLds {
  int cnt[SAMPLE_V];            // occurrences of every byte in the window
  unsigned key[SAMPLE_V];       // the logits as unsigned keys of one total order (NaN included): the rank is a permutation
  float srt[SAMPLE_V];          // exp(l - max) in descending order of l
  float part[SAMPLE_WAVES];     // wavefront totals of the reduction / scan in flight
  float pick;                   // the top_k-th largest value
  int run, first, last;
};

// inclusive scan of v over the workgroup in thread order; *total = the sum of all (the same association for every
// thread: the wavefront totals added in wavefront order)
__device__ __forceinline__ float block_scan(float v, SampleLds& sm, float* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  __syncthreads();                               // the previous user of part[] is done
  if (lane == 63) sm.part[wv] = v;
  __syncthreads();
  float before = 0.f, all = 0.f;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) {
    if (w == wv) before = all;
    all += sm.part[w];
  }
  *total = all;
  return wv == 0 ? v : before + v;
}

__device__ __forceinline__ float block_max(float v, SampleLds& sm) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm.part[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = sm.part[0];
#pragma unroll
  for (int w = 1; w < SAMPLE_WAVES; ++w) m = fmaxf(m, sm.part[w]);
  return m;
}

// descending order of the floats = descending order of these keys; -0 and +0 share a key (equal logits are ordered by
// index), a NaN sorts above or below everything by its sign: whatever the row holds, the ranks are a permutation
__device__ __forceinline__ unsigned order_key(float x) {
  if (x == 0.f) return 0x80000000u;
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename TOK>
__global__ __launch_bounds__(SAMPLE_V) void k_sample_bytes(const float* __restrict__ logits, long long row_stride,
                                                           const TOK* __restrict__ recent, int n_recent, SampleArgs a,
                                                           const float* __restrict__ u, long long* __restrict__ ids,
                                                           float* __restrict__ probs) {
  __shared__ SampleLds sm;
  const int t = threadIdx.x;
  const size_t r = blockIdx.x;
  const float ninf = -__builtin_huge_valf();
  float l = logits[r * (size_t)row_stride + t];                                          // step 1
  sm.cnt[t] = 0;
  if (t == 0) { sm.run = 1; sm.first = SAMPLE_V; sm.last = -1; sm.pick = ninf; }
  __syncthreads();
  for (int i = t; i < n_recent; i += SAMPLE_V) {
    const long long b = (long long)recent[i];
    if (b >= 0 && b < SAMPLE_V) atomicAdd(&sm.cnt[(int)b], 1);                           // (LDS, integers: exact)
  }
  const bool run_on = a.max_run > 0 && n_recent >= a.max_run;
  long long run_byte = -1;
  if (run_on) {
    run_byte = (long long)recent[n_recent - 1];
    for (int i = t; i < a.max_run; i += SAMPLE_V)
      if ((long long)recent[n_recent - 1 - i] != run_byte) sm.run = 0;                   // (every writer stores the same 0)
  }
  __syncthreads();
  const int c = sm.cnt[t];
  if (c > 0) {
    l = l / a.rep;                                                                       // step 2
    if (a.presence != 0.f || a.frequency != 0.f) l = l - a.presence - a.frequency * (float)c;   // step 3
  }
  if (a.ascii_only && !(t == 10 || (t >= 32 && t <= 126))) l = ninf;                     // step 4
  if (a.ban_cr && t == 13) l = ninf;
  if (run_on && sm.run && run_byte == t) l = ninf;                                       // step 5
  l = l / a.temperature;                                                                 // step 6
  const bool nucleus = a.top_p < 1.f;
  const int kk = a.top_k > SAMPLE_V ? SAMPLE_V : a.top_k;
  if (nucleus || kk > 0) {
    // the descending rank of l, ties by index: SAMPLE_V broadcast reads of the keys
    const unsigned key = order_key(l);
    sm.key[t] = key;
    __syncthreads();
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < SAMPLE_V; ++j) {
      const unsigned kj = sm.key[j];
      rank += (kj > key || (kj == key && j < t)) ? 1 : 0;
    }
    int kept = SAMPLE_V;
    if (nucleus) {                                                                       // step 7
      const float m = block_max(l, sm);
      sm.srt[rank] = expf(l - m);
      __syncthreads();
      const float e = sm.srt[t];
      float sum;
      block_scan(e, sm, &sum);
      float unused;
      const float cdf = block_scan(e / sum, sm, &unused);                                // running sum of the sorted softmax
      kept = __syncthreads_count(cdf <= a.top_p || t == 0);
      if (rank >= kept) l = ninf;
    }
    if (kk > 0) {                                                                        // step 8
      if (rank == kk - 1 && kk <= kept) sm.pick = l;      // (past the nucleus: -inf, which is below nothing)
      __syncthreads();
      if (l < sm.pick) l = ninf;
    }
  }
  const float m = block_max(l, sm);                                                      // step 9
  const float e = expf(l - m);
  float sum;
  block_scan(e, sm, &sum);
  const float p = e / sum;
  float unused;
  const float cum = block_scan(p, sm, &unused);                                          // step 10
  if (probs) probs[r * SAMPLE_V + t] = p;
  // the first index whose running sum exceeds u, among the bytes that can be drawn at all; where rounding leaves u above
  // the last running sum, the last such byte; a row without any (NaN logits): 0
  if (p > 0.f) {
    atomicMax(&sm.last, t);
    if (cum > u[r]) atomicMin(&sm.first, t);
  }
  __syncthreads();
  if (t == 0) ids[r] = sm.first < SAMPLE_V ? sm.first : (sm.last >= 0 ? sm.last : 0);
}

}  // namespace

hipError_t launch_sample_bytes(const float* logits, long long row_stride, const void* recent, int kind, int n_recent,
                               const SampleArgs& a, const float* u, long long* ids, float* probs, long long R,
                               hipStream_t s) {
  if (R < 1 || R > 0x7fffffffll || row_stride < SAMPLE_V || n_recent < 0 || n_recent > SAMPLE_MAX_RECENT)
    return hipErrorInvalidValue;
  if (kind == 1)
    hipLaunchKernelGGL(k_sample_bytes<unsigned char>, dim3((unsigned)R), dim3(SAMPLE_V), 0, s, logits, row_stride,
                       (const unsigned char*)recent, n_recent, a, u, ids, probs);
  else
    hipLaunchKernelGGL(k_sample_bytes<long long>, dim3((unsigned)R), dim3(SAMPLE_V), 0, s, logits, row_stride,
                       (const long long*)recent, n_recent, a, u, ids, probs);
  return hipGetLastError();
}

}  // namespace smx
