// smx_sst.hip -- the two native ops of the sparse spectral tensor (reference fft_tensor/tensor.py): the top-k sparsify of
// a complex64 spectrum (_sparsify_pytorch, :136-144: abs, topk -- a sort --, >=, nonzero, masked gather) and the scatter
// back to a dense spectrum (_scatter_pytorch, :194-203: fill + index_put).  The reference's setup.py declares both as an
// extension whose sources were never written.
//
// Definition (numpy reproduces it bit for bit).  For n complex64 values z[i] = (re, im):
//   key[i] = bits(fl(fl(re re) + fl(im im))) & 0x7fffffff      fp32, round to nearest, no FMA; compared as unsigned
//   T      = the k-th largest key, 1 <= k <= n;   kept = {i : key[i] >= T}, m = |kept| >= k (ties at T are all kept)
//   coeffs[j], flat_idx[j] = z and index of the j-th kept element in ascending index order (torch.nonzero's order).
// A NaN key (0x7fc00000 and up) ranks above inf.
//
// Coordinates.  z is 8-byte aligned; with off = ((address of z) mod 16) / 8, q = i + off counts elements from the 16-byte
// boundary below z, pair p holds q = 2p, 2p + 1, and tile t the positions q in [t * 4096, (t + 1) * 4096): a pair wholly
// inside [z, z + n) is ONE 16-byte load, a pair cut by either end is read element by element (nothing outside is read).
//
// Selection: an exact radix select over the 31 key bits in THREE passes over the spectrum (digits of 11, 10 and 10 bits,
// from the top).  Per pass k_topk_hist: G persistent workgroups walk tiles g, g + G, ... and count, in an LDS histogram
// (integer LDS atomics), the digit of every key whose higher bits equal the prefix found so far; each writes its
// histogram as row g of a (G, bins) table.  k_topk_join sums the columns; k_topk_pick (one workgroup) takes the digit that
// holds the remaining rank, extends the prefix, lowers the rank and counts the keys above.  After the third pick T and m
// are on the device.  k_topk_count then counts the kept elements per tile (a fourth read), k_topk_scan turns the counts
// into offsets (one workgroup), and smx_topk_compact's k_topk_write (a fifth read) places every kept element at
// offset[tile] + its rank inside the tile (ballots per wave round, a 32-entry prefix per tile).
//
// Scatter: one launch.  A workgroup owns a CONTIGUOUS run of 4096-element tiles of `out`; it finds its first entry by
// binary search in flat_idx, then per tile zeroes an LDS image, drops the tile's entries into it (walking flat_idx
// forward, 256 entries a round) and stores the image with 16-byte stores: `out` is written exactly once, nothing of
// size n is read.  An index outside the tile is never used as an address, so a broken promise (unordered or out-of-range
// flat_idx) gives unspecified contents of `out` and touches nothing else.
//
// No flag words, no waiting of one workgroup on another, no atomics on global memory, nothing allocated, no host
// synchronisation: integer counts do not depend on order, so every result is a pure function of the inputs.
//
// The launchers and size rules at the end of this file are declared in smx_kernels.h; the C entries are in smx_api.hip.
#include <cstdint>

#include "smx_kernels.h"

namespace smx {

constexpr int SST_BLOCK = 256;
constexpr int SST_TILE = 4096;                            // elements per tile (32 KiB of spectrum)
constexpr int SST_PAIRS = SST_TILE / 2;                   // 16-byte pairs per tile
constexpr int SST_ROUNDS = SST_PAIRS / SST_BLOCK;         // 8 pairs per thread and tile
constexpr int SST_WAVES = SST_BLOCK / 64;
constexpr int SST_SEGS = SST_ROUNDS * SST_WAVES;          // 32 wave rounds per tile, 128 consecutive elements each
constexpr int TOPK_BITS0 = 11, TOPK_BITS1 = 10, TOPK_BITS2 = 10;
constexpr int TOPK_MAX_BINS = 1 << TOPK_BITS0;            // 2048
constexpr int TOPK_HIST_WG = 512;                         // histogram rows at most (2 workgroups per CU)
constexpr int TOPK_WALK_WG = 1024;                        // count / write workgroups at most
constexpr int TOPK_JOIN_BINS = 16, TOPK_JOIN_GROUPS = SST_BLOCK / TOPK_JOIN_BINS;
constexpr int SCATTER_WG = 2048;
constexpr long long SST_MAX_N = (1ll << 31) - 1;

// Two products and a sum, each rounded.  build.sh compiles the other units with -ffp-contract=fast, under which the
// backend fuses any product into a following sum -- HIP's __fmul_rn / __fadd_rn are plain `*` and `+` in a header, and
// `#pragma clang fp contract(off)` is ignored by that mode -- and it fused differently from kernel to kernel (seen on the
// device: fma(re, re, fl(im im)) in one, fma(im, im, fl(re re)) in another, keys one ulp apart).  This unit is therefore
// compiled with -ffp-contract=off (build.sh); it holds no other floating-point arithmetic.
__device__ __forceinline__ unsigned topk_key(float2 v) {
  const float rr = v.x * v.x;
  const float ii = v.y * v.y;
  return __float_as_uint(rr + ii) & 0x7fffffffu;
}

// pair p of the coordinates above: elements i0 = 2p - off and i0 + 1; va / vb say which of them exist
__device__ __forceinline__ void topk_load_pair(const TopkArgs& a, long long p, float2& ea, float2& eb, bool& va, bool& vb) {
  const long long i0 = 2 * p - a.off;
  if (i0 >= 0 && i0 + 1 < a.n) {
    const float4 v = *reinterpret_cast<const float4*>(a.z + i0);     // (z - off) + 2p elements: 16-byte aligned
    ea = make_float2(v.x, v.y); eb = make_float2(v.z, v.w);
    va = vb = true;
    return;
  }
  va = i0 >= 0 && i0 < a.n;
  vb = i0 + 1 >= 0 && i0 + 1 < a.n;
  ea = va ? a.z[i0] : make_float2(0.f, 0.f);
  eb = vb ? a.z[i0 + 1] : make_float2(0.f, 0.f);
}

// One pass of the radix select.  shift / bits: the digit is (key >> shift) & (2^bits - 1); the keys counted are those
// with key >> (shift + bits) == state->prefix (every key in the first pass: state == nullptr).
__global__ __launch_bounds__(SST_BLOCK) void k_topk_hist(TopkArgs a, const TopkState* __restrict__ state, int shift, int bits,
                                                         unsigned* __restrict__ rows) {
  __shared__ unsigned hist[TOPK_MAX_BINS];
  const int tid = threadIdx.x, nb = 1 << bits;
  for (int i = tid; i < nb; i += SST_BLOCK) hist[i] = 0u;
  const bool all = state == nullptr;
  const unsigned prefix = all ? 0u : state->prefix;
  const unsigned mask = (unsigned)nb - 1u;
  const int hi = shift + bits;                            // <= 31; 31 in the first pass, where every key matches
  __syncthreads();
  for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
#pragma unroll
    for (int r = 0; r < SST_ROUNDS; ++r) {
      float2 ea, eb; bool va, vb;
      topk_load_pair(a, t * SST_PAIRS + r * SST_BLOCK + tid, ea, eb, va, vb);
      const unsigned ka = topk_key(ea), kb = topk_key(eb);
      if (va && (all || (ka >> hi) == prefix)) atomicAdd(&hist[(ka >> shift) & mask], 1u);
      if (vb && (all || (kb >> hi) == prefix)) atomicAdd(&hist[(kb >> shift) & mask], 1u);
    }
  }
  __syncthreads();
  unsigned* row = rows + (size_t)blockIdx.x * nb;
  for (int i = tid; i < nb; i += SST_BLOCK) row[i] = hist[i];
}

// totals[b] = sum over the G rows of column b.  A workgroup takes 16 columns; its 256 threads are 16 row groups.
__global__ __launch_bounds__(SST_BLOCK) void k_topk_join(const unsigned* __restrict__ rows, int G, int nb,
                                                         unsigned* __restrict__ totals) {
  __shared__ unsigned part[TOPK_JOIN_GROUPS][TOPK_JOIN_BINS];
  const int c = threadIdx.x % TOPK_JOIN_BINS, rg = threadIdx.x / TOPK_JOIN_BINS;
  const int b = blockIdx.x * TOPK_JOIN_BINS + c;          // nb is a multiple of 16
  unsigned s = 0u;
#pragma unroll 8
  for (int g = rg; g < G; g += TOPK_JOIN_GROUPS) s += rows[(size_t)g * nb + b];
  part[rg][c] = s;
  __syncthreads();
  if (rg == 0) {
#pragma unroll
    for (int j = 1; j < TOPK_JOIN_GROUPS; ++j) s += part[j][c];
    totals[b] = s;
  }
}

// The digit d of this pass: the largest d with S(d) = sum of totals[d ...] >= rank.  One workgroup; thread t owns the
// nb / 256 bins from t * per.  first: rank = k, no prefix yet.  last: result[0] = m, result[1] = T.
__global__ __launch_bounds__(SST_BLOCK) void k_topk_pick(const unsigned* __restrict__ totals, int bits, unsigned k, int first,
                                                         int last, TopkState* __restrict__ state, long long* __restrict__ result) {
  __shared__ unsigned suf[SST_BLOCK];
  const int tid = threadIdx.x, per = (1 << bits) / SST_BLOCK;          // 8 or 4
  const unsigned rank = first ? k : state->rank, prefix = first ? 0u : state->prefix, above = first ? 0u : state->above;
  unsigned own = 0u;
  for (int j = 0; j < per; ++j) own += totals[tid * per + j];
  suf[tid] = own;
  __syncthreads();                                        // (also: every thread has read *state before it is rewritten)
  for (int d = 1; d < SST_BLOCK; d <<= 1) {               // inclusive suffix sums: suf[t] = sum of own[t ...]
    const unsigned add = tid + d < SST_BLOCK ? suf[tid + d] : 0u;
    __syncthreads();
    suf[tid] += add;
    __syncthreads();
  }
  const unsigned incl = suf[tid], excl = incl - own;
  if (excl < rank && rank <= incl) {                      // exactly one thread: suffix sums fall with t, 1 <= rank <= suf[0]
    unsigned higher = excl;                               // keys in bins above the one looked at
    int d = tid * per + per - 1;
    for (;; --d) {
      const unsigned c = totals[d];
      if (higher + c >= rank) break;                      // reached at the latest at d = tid * per, where higher + c = incl
      higher += c;
    }
    const unsigned np = (prefix << bits) | (unsigned)d;
    state->prefix = np;
    state->rank = rank - higher;
    state->above = above + higher;
    if (last) {
      result[0] = (long long)(above + higher) + (long long)totals[d];
      result[1] = (long long)np;
    }
  }
}

// counts[t] = kept elements (key >= T) of tile t
__global__ __launch_bounds__(SST_BLOCK) void k_topk_count(TopkArgs a, const long long* __restrict__ result,
                                                          unsigned* __restrict__ counts) {
  __shared__ unsigned wsum[SST_WAVES];
  const int tid = threadIdx.x;
  const unsigned T = (unsigned)result[1];
  for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    unsigned c = 0u;
#pragma unroll
    for (int r = 0; r < SST_ROUNDS; ++r) {
      float2 ea, eb; bool va, vb;
      topk_load_pair(a, t * SST_PAIRS + r * SST_BLOCK + tid, ea, eb, va, vb);
      c += (va && topk_key(ea) >= T) ? 1u : 0u;
      c += (vb && topk_key(eb) >= T) ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    __syncthreads();                                      // the previous tile's sums have been read
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
      unsigned s = 0u;
#pragma unroll
      for (int w = 0; w < SST_WAVES; ++w) s += wsum[w];
      counts[t] = s;
    }
  }
}

// counts -> exclusive prefix sums, in place.  One workgroup of 1024 threads, a contiguous chunk of tiles per thread.
__global__ __launch_bounds__(1024) void k_topk_scan(unsigned* __restrict__ counts, long long ntiles) {
  __shared__ unsigned sums[1024];
  const int tid = threadIdx.x;
  const long long per = (ntiles + 1023) / 1024;
  const long long lo = tid * per, hi = lo + per < ntiles ? lo + per : ntiles;
  unsigned own = 0u;
  for (long long i = lo; i < hi; ++i) own += counts[i];
  sums[tid] = own;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {                    // inclusive prefix sums over the threads
    const unsigned add = tid >= d ? sums[tid - d] : 0u;
    __syncthreads();
    sums[tid] += add;
    __syncthreads();
  }
  unsigned run = sums[tid] - own;
  for (long long i = lo; i < hi; ++i) {
    const unsigned c = counts[i];
    counts[i] = run;
    run += c;
  }
}

// The write pass: element order inside a tile is (round r, wave w, lane, first / second of the pair) = ascending index,
// so the rank of a kept element is: kept in earlier wave rounds + kept in lower lanes of this one (two ballots).
__global__ __launch_bounds__(SST_BLOCK) void k_topk_write(TopkArgs a, const long long* __restrict__ result,
                                                          const unsigned* __restrict__ offsets, float2* __restrict__ coeffs,
                                                          long long* __restrict__ flat_idx, long long capacity) {
  __shared__ unsigned seg[SST_SEGS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned T = (unsigned)result[1];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const long long base = offsets[t];
    if (base >= capacity) continue;                       // the same for the whole workgroup
    float2 ea[SST_ROUNDS], eb[SST_ROUNDS];
    unsigned ra[SST_ROUNDS], rb[SST_ROUNDS];              // rank inside the wave round; ~0u: not kept
    __syncthreads();                                      // the previous tile's seg[] has been read
#pragma unroll
    for (int r = 0; r < SST_ROUNDS; ++r) {
      bool va, vb;
      topk_load_pair(a, t * SST_PAIRS + r * SST_BLOCK + tid, ea[r], eb[r], va, vb);
      const bool ka = va && topk_key(ea[r]) >= T, kb = vb && topk_key(eb[r]) >= T;
      const unsigned long long ba = __ballot(ka), bb = __ballot(kb);
      const unsigned before = (unsigned)__popcll(ba & below) + (unsigned)__popcll(bb & below);
      ra[r] = ka ? before : ~0u;
      rb[r] = kb ? before + (ka ? 1u : 0u) : ~0u;
      if (lane == 0) seg[r * SST_WAVES + wave] = (unsigned)__popcll(ba) + (unsigned)__popcll(bb);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SST_ROUNDS; ++r) {
      const int s = r * SST_WAVES + wave;
      unsigned pre = 0u;
      for (int j = 0; j < s; ++j) pre += seg[j];
      const long long i0 = 2 * (t * SST_PAIRS + r * SST_BLOCK + tid) - a.off;
      if (ra[r] != ~0u) {
        const long long pos = base + pre + ra[r];
        if (pos < capacity) { coeffs[pos] = ea[r]; flat_idx[pos] = i0; }
      }
      if (rb[r] != ~0u) {
        const long long pos = base + pre + rb[r];
        if (pos < capacity) { coeffs[pos] = eb[r]; flat_idx[pos] = i0 + 1; }
      }
    }
  }
}

// out = zeros, out[flat_idx[j]] = coeffs[j].  Workgroup g owns tiles [g * per, (g + 1) * per).
__global__ __launch_bounds__(SST_BLOCK) void k_sparse_scatter(const float2* __restrict__ coeffs,
                                                              const long long* __restrict__ flat_idx, long long m,
                                                              float2* __restrict__ out, long long n, long long ntiles,
                                                              long long per) {
  __shared__ __align__(16) float2 image[SST_TILE];
  __shared__ long long s_next;
  const int tid = threadIdx.x;
  const long long t0 = blockIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  long long cur = 0;                                      // the first entry at or after the first owned element
  {
    const long long first = t0 * SST_TILE;
    long long lo = 0, hi = m;
    while (lo < hi) {
      const long long mid = lo + (hi - lo) / 2;
      if (flat_idx[mid] < first) lo = mid + 1; else hi = mid;
    }
    cur = lo;
  }
  float4* img4 = reinterpret_cast<float4*>(image);
  for (long long t = t0; t < t1; ++t) {
    const long long start = t * SST_TILE, end = start + SST_TILE < n ? start + SST_TILE : n;
    __syncthreads();                                      // the previous tile's image and s_next have been read
    for (int i = tid; i < SST_PAIRS; i += SST_BLOCK) img4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid == 0) s_next = cur;
    __syncthreads();
    for (long long j0 = cur; j0 < m; j0 += SST_BLOCK) {   // j0 and the exit test are the same for every thread
      const long long j = j0 + tid;
      if (j < m) {
        const long long idx = flat_idx[j];
        if (idx >= start && idx < end) {                  // only such an index becomes an address
          image[idx - start] = coeffs[j];
          if (j + 1 == m || flat_idx[j + 1] >= end) s_next = j + 1;      // the tile's last entry (one thread when ascending)
        }
      }
      const long long jl = j0 + SST_BLOCK - 1;
      if (jl >= m || flat_idx[jl] >= end) break;
    }
    __syncthreads();
    cur = s_next;                                         // > the old cur or unchanged; never beyond m
    const long long len = end - start;
    float4* o4 = reinterpret_cast<float4*>(out + start);  // out is 16-byte aligned, start a multiple of 4096
    for (int i = tid; i < SST_PAIRS; i += SST_BLOCK) {
      if (2ll * i + 1 < len) o4[i] = img4[i];
      else if (2ll * i < len) out[start + 2 * i] = image[2 * i];
    }
  }
}

bool topk_supported(long long n) { return n >= 1 && n <= SST_MAX_N; }

// workspace: state | totals (2048) | rows (min(512, tiles), 2048) | tile counts / offsets
TopkLayout topk_layout(long long n) {
  const long long tiles = (n + 1 + SST_TILE - 1) / SST_TILE;                 // off is 0 or 1
  const long long g = tiles < TOPK_HIST_WG ? tiles : TOPK_HIST_WG;
  TopkLayout l;
  l.totals = al(sizeof(TopkState));
  l.rows = l.totals + al((size_t)TOPK_MAX_BINS * 4);
  l.counts = l.rows + al((size_t)g * TOPK_MAX_BINS * 4);
  l.need = l.counts + al((size_t)tiles * 4);
  return l;
}

namespace {

TopkArgs topk_args(const float2* z, long long n) {
  TopkArgs a{};
  a.z = z; a.n = n;
  a.off = (int)(((uintptr_t)z & 15) / 8);
  a.ntiles = (a.off + n + SST_TILE - 1) / SST_TILE;
  return a;
}

}  // namespace

hipError_t launch_topk_select(const float2* z, long long n, long long k, long long* result, void* workspace,
                              int max_workgroups, hipStream_t s) {
  const TopkArgs a = topk_args(z, n);
  const TopkLayout l = topk_layout(n);
  char* ws = (char*)workspace;
  TopkState* state = (TopkState*)ws;
  unsigned* totals = (unsigned*)(ws + l.totals);
  unsigned* rows = (unsigned*)(ws + l.rows);
  unsigned* counts = (unsigned*)(ws + l.counts);
  const int G = tile_workgroups(a.ntiles, TOPK_HIST_WG, max_workgroups);      // <= min(512, tiles): the rows fit
  const int Gw = tile_workgroups(a.ntiles, TOPK_WALK_WG, max_workgroups);
  const int bits[3] = {TOPK_BITS0, TOPK_BITS1, TOPK_BITS2};
  int shift = 31;
  for (int p = 0; p < 3; ++p) {
    shift -= bits[p];
    const int nb = 1 << bits[p];
    hipLaunchKernelGGL(k_topk_hist, dim3((unsigned)G), dim3(SST_BLOCK), 0, s, a, p == 0 ? (const TopkState*)nullptr : state,
                       shift, bits[p], rows);
    hipLaunchKernelGGL(k_topk_join, dim3((unsigned)(nb / TOPK_JOIN_BINS)), dim3(SST_BLOCK), 0, s, (const unsigned*)rows, G, nb,
                       totals);
    hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(SST_BLOCK), 0, s, (const unsigned*)totals, bits[p], (unsigned)k,
                       p == 0 ? 1 : 0, p == 2 ? 1 : 0, state, result);
  }
  hipLaunchKernelGGL(k_topk_count, dim3((unsigned)Gw), dim3(SST_BLOCK), 0, s, a, (const long long*)result, counts);
  hipLaunchKernelGGL(k_topk_scan, dim3(1), dim3(1024), 0, s, counts, a.ntiles);
  return hipGetLastError();
}

hipError_t launch_topk_compact(const float2* z, long long n, const long long* result, float2* coeffs, long long* flat_idx,
                               long long capacity, const void* workspace, int max_workgroups, hipStream_t s) {
  const TopkArgs a = topk_args(z, n);
  const unsigned* offsets = (const unsigned*)((const char*)workspace + topk_layout(n).counts);
  const int Gw = tile_workgroups(a.ntiles, TOPK_WALK_WG, max_workgroups);
  hipLaunchKernelGGL(k_topk_write, dim3((unsigned)Gw), dim3(SST_BLOCK), 0, s, a, result, offsets, coeffs, flat_idx, capacity);
  return hipGetLastError();
}

hipError_t launch_sparse_scatter(const float2* coeffs, const long long* flat_idx, long long m, float2* out, long long n,
                                 int max_workgroups, hipStream_t s) {
  const long long ntiles = (n + SST_TILE - 1) / SST_TILE;
  const int G = tile_workgroups(ntiles, SCATTER_WG, max_workgroups);
  const long long per = (ntiles + G - 1) / G;
  hipLaunchKernelGGL(k_sparse_scatter, dim3((unsigned)G), dim3(SST_BLOCK), 0, s, coeffs, flat_idx, m, out, n, ntiles, per);
  return hipGetLastError();
}

}  // namespace smx
