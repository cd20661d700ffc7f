// smx_match.hip -- multi-pattern exact byte search: the `corpus_bytes.find(snip)` loop of the trainer's parroting score
// (reference fft_lm/train_fixed_full.py:185-205, up to 64 host scans of the whole corpus per epoch) as ONE pass over the
// corpus that tests every snippet at every position, and a small launch that joins the workgroups' answers.
//
// first[s] = the smallest p in [0, n - L] with corpus[p : p + L] == snips[s], -1 when there is none (bytes.find).
//
// Coordinates.  With off = (address of corpus) mod 16, q = p + off is a position counted from the 16-byte boundary below
// the corpus; tile t holds the positions q in [t * 16384, (t + 1) * 16384), so every tile starts on a 16-byte address
// whatever the alignment of the corpus (the first tile is `off` positions short).  A workgroup owns tiles g, g + G, ...
// of G persistent workgroups and keeps, in LDS,
//   image   the tile's bytes and a halo of L - 1 more, as 16-byte vectors: a vector wholly inside [corpus, corpus + n) is
//           ONE 16-byte load, a vector that crosses either end is read byte by byte (bytes outside are never read: zero);
//           the next tile's vectors are loaded into registers before the current tile is scanned;
//   snips   the S * L snippet bytes (dynamic LDS, so that a small set leaves room for more workgroups per CU);
//   bitmap  65536 bits over a 16-bit hash of each snippet's first four bytes: a thread forms the sixteen 4-byte windows of
//           its 16 image bytes in registers (one 16-byte and one 4-byte LDS read), looks each up, and only for a set bit
//   head / next / fw   walks the chain of the snippets in that hash bucket, compares the window with the snippet's first
//           word and then the remaining L - 4 bytes from LDS, leaving at the first mismatch;
//   best    the smallest position found so far per snippet (64-bit LDS minimum).  A candidate at or above best[s] is not
//           verified: a corpus of one repeated byte verifies a matching snippet once per thread, not once per position.
// The workgroup's S minima go to row g of a (G, S) table in the workspace; k_match_join takes the minimum of each
// column, one workgroup per snippet.  No flag words, no waiting of one workgroup on another, no global atomics: a minimum does not
// depend on the order in which positions are found, so the answer is a pure function of the inputs.
//
// The launcher and size rules at the end of this file are declared in smx_kernels.h; the C entries are in smx_api.hip.
#include <cstdint>

#include "smx_kernels.h"

namespace smx {

constexpr int MATCH_BLOCK = 256;
constexpr int MATCH_TILE = 16384;                         // positions per tile
constexpr int MATCH_MAX_S = 256, MATCH_MAX_L = 256, MATCH_MAX_BYTES = 32768;
constexpr int MATCH_IMAGE_VECS = (MATCH_TILE + MATCH_MAX_L - 1 + 15) / 16;      // 1040
constexpr int MATCH_FULL_VECS = MATCH_TILE / 16;          // 1024 = 4 per thread
constexpr int MATCH_VEC_REGS = (MATCH_IMAGE_VECS + MATCH_BLOCK - 1) / MATCH_BLOCK;   // 5 per thread
constexpr int MATCH_HASH_BITS = 16, MATCH_BUCKET_BITS = 9;
constexpr int MATCH_BITMAP_WORDS = (1 << MATCH_HASH_BITS) / 32;
constexpr int MATCH_BUCKETS = 1 << MATCH_BUCKET_BITS;
constexpr int MATCH_CUS = 256, MATCH_MAX_WG = 4 * MATCH_CUS;
constexpr int MATCH_STATIC_LDS = MATCH_IMAGE_VECS * 16 + MATCH_BITMAP_WORDS * 4 + MATCH_BUCKETS * 4
                                 + MATCH_MAX_S * (4 + 4 + 8);
constexpr unsigned long long MATCH_NONE = ~0ull;

SMX_HD unsigned match_hash(unsigned w) { return (w * 0x9E3779B1u) >> (32 - MATCH_HASH_BITS); }

// the 16 bytes at corpus index `idx` (a multiple of 16 in address terms; may start before 0 or end after n)
__device__ __forceinline__ uint4 match_load_vec(const unsigned char* corpus, long long n, long long idx) {
  if (idx >= 0 && idx + 16 <= n) return *reinterpret_cast<const uint4*>(corpus + idx);
  unsigned w[4] = {0u, 0u, 0u, 0u};
  if (idx + 16 > 0 && idx < n) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long long k = idx + j;
      if (k >= 0 && k < n) w[j >> 2] |= (unsigned)corpus[k] << (8 * (j & 3));
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(MATCH_BLOCK) void k_match_scan(MatchArgs a) {
  __shared__ __align__(16) uint4 image[MATCH_IMAGE_VECS];
  __shared__ unsigned bitmap[MATCH_BITMAP_WORDS];
  __shared__ int head[MATCH_BUCKETS];
  __shared__ int next[MATCH_MAX_S];
  __shared__ unsigned fw[MATCH_MAX_S];
  __shared__ unsigned long long best[MATCH_MAX_S];
  extern __shared__ __align__(16) unsigned char snl[];    // S * L snippet bytes
  const int tid = threadIdx.x, S = a.S, L = a.L;
  const long long G = gridDim.x;

  for (int i = tid; i < MATCH_BITMAP_WORDS; i += MATCH_BLOCK) bitmap[i] = 0u;
  for (int i = tid; i < MATCH_BUCKETS; i += MATCH_BLOCK) head[i] = -1;
  for (int i = tid; i < S * L; i += MATCH_BLOCK) snl[i] = a.snips[i];
  if (tid < S) best[tid] = MATCH_NONE;
  __syncthreads();
  if (tid < S) {
    const unsigned char* sp = snl + tid * L;
    const unsigned w = (unsigned)sp[0] | ((unsigned)sp[1] << 8) | ((unsigned)sp[2] << 16) | ((unsigned)sp[3] << 24);
    const unsigned h = match_hash(w);
    fw[tid] = w;
    atomicOr(&bitmap[h >> 5], 1u << (h & 31));
    next[tid] = atomicExch(&head[h >> (MATCH_HASH_BITS - MATCH_BUCKET_BITS)], tid);   // chain order is free: a minimum
  }

  const long long qlo = a.off, qhi = a.off + a.npos;      // valid positions q (p = q - off)
  uint4 reg[MATCH_VEC_REGS];
  long long t = blockIdx.x;
  if (t < a.ntiles) {
#pragma unroll
    for (int i = 0; i < MATCH_VEC_REGS; ++i) {
      const int v = tid + i * MATCH_BLOCK;
      reg[i] = v < a.nvec ? match_load_vec(a.corpus, a.n, t * MATCH_TILE + 16ll * v - a.off) : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  for (; t < a.ntiles; t += G) {
    __syncthreads();                                      // the set-up above / the previous tile's scan is over
#pragma unroll
    for (int i = 0; i < MATCH_VEC_REGS; ++i) {
      const int v = tid + i * MATCH_BLOCK;
      if (v < a.nvec) image[v] = reg[i];
    }
    __syncthreads();
    if (t + G < a.ntiles) {
#pragma unroll
      for (int i = 0; i < MATCH_VEC_REGS; ++i) {
        const int v = tid + i * MATCH_BLOCK;
        reg[i] = v < a.nvec ? match_load_vec(a.corpus, a.n, (t + G) * MATCH_TILE + 16ll * v - a.off)
                            : make_uint4(0u, 0u, 0u, 0u);
      }
    }
    const long long q0 = t * MATCH_TILE;
    const unsigned char* img = reinterpret_cast<const unsigned char*>(image);
    const unsigned* img32 = reinterpret_cast<const unsigned*>(image);
#pragma unroll 1
    for (int c = tid; c < MATCH_FULL_VECS; c += MATCH_BLOCK) {
      if (q0 + 16ll * c >= qhi) break;                    // nothing valid from here on (ascending in c)
      const uint4 x = image[c];
      const unsigned w[5] = {x.x, x.y, x.z, x.w, img32[4 * c + 4]};   // vector c + 1 exists: nvec > MATCH_FULL_VECS
      unsigned hits = 0u;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = j & 3;
        const unsigned win = k == 0 ? w[j >> 2] : (w[j >> 2] >> (8 * k)) | (w[(j >> 2) + 1] << (32 - 8 * k));
        const unsigned h = match_hash(win);
        hits |= ((bitmap[h >> 5] >> (h & 31)) & 1u) << j;
      }
      while (hits) {
        const int j = __ffs(hits) - 1;
        hits &= hits - 1u;
        const int lp = 16 * c + j;                        // image index of the position
        const long long q = q0 + lp;
        if (q < qlo || q >= qhi) continue;                // before the corpus / a window cut off by its end
        const unsigned long long p = (unsigned long long)(q - qlo);
        const unsigned char* ip = img + lp;
        const unsigned win = (unsigned)ip[0] | ((unsigned)ip[1] << 8) | ((unsigned)ip[2] << 16) | ((unsigned)ip[3] << 24);
        for (int s = head[match_hash(win) >> (MATCH_HASH_BITS - MATCH_BUCKET_BITS)]; s >= 0; s = next[s]) {
          if (fw[s] != win) continue;
          if (p >= __hip_atomic_load(&best[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;
          const unsigned char* sp = snl + s * L;
          int k = 4;
          while (k < L && sp[k] == ip[k]) ++k;            // lp + L - 1 < 16 nvec for every valid q
          if (k == L) atomicMin(&best[s], p);
        }
      }
    }
  }
  __syncthreads();
  if (tid < S) a.part[(size_t)blockIdx.x * S + tid] = best[tid];
}

// first[s] = min over the G rows of column s of part, -1 when no workgroup found snippet s (G = 0: n < L).  One
// workgroup per snippet: thread j takes rows j, j + 256, ... (independent loads: one thread walking all rows pays a memory
// latency per row, 0.25 ms at 1024 rows), then a tree over LDS.  A minimum: the same in any order.
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_join(const unsigned long long* __restrict__ part,
                                                           long long* __restrict__ first, int G, int S) {
  __shared__ unsigned long long red[MATCH_BLOCK];
  const int s = blockIdx.x, tid = threadIdx.x;
  unsigned long long m = MATCH_NONE;
  for (int g = tid; g < G; g += MATCH_BLOCK) {
    const unsigned long long v = part[(size_t)g * S + s];
    m = v < m ? v : m;
  }
  red[tid] = m;
  __syncthreads();
  for (int d = MATCH_BLOCK / 2; d > 0; d >>= 1) {
    if (tid < d) red[tid] = red[tid + d] < red[tid] ? red[tid + d] : red[tid];
    __syncthreads();
  }
  if (tid == 0) first[s] = red[0] == MATCH_NONE ? -1ll : (long long)red[0];
}

bool match_supported(int S, int L) {
  return S >= 1 && S <= MATCH_MAX_S && L >= 4 && L <= MATCH_MAX_L && (long long)S * L <= MATCH_MAX_BYTES;
}
size_t match_part_bytes(int S) { return al((size_t)MATCH_MAX_WG * S * sizeof(unsigned long long)); }

hipError_t launch_match_first(const unsigned char* corpus, long long n, const unsigned char* snips, int S, int L,
                              long long* first, unsigned long long* part, int max_workgroups, hipStream_t s) {
  MatchArgs a{};
  a.corpus = corpus; a.snips = snips; a.part = part;
  a.n = n; a.npos = n - L + 1; a.S = S; a.L = L;
  a.off = (int)((uintptr_t)corpus & 15);
  a.nvec = (MATCH_TILE + L - 1 + 15) / 16;
  a.ntiles = a.npos > 0 ? (a.off + a.npos + MATCH_TILE - 1) / MATCH_TILE : 0;
  // as many workgroups as stay resident: LDS bounds them to 2 ... 4 per CU (`max_workgroups`: tests, 1 or 2)
  const int lds = MATCH_STATIC_LDS + (S * L + 15) / 16 * 16;
  int per_cu = (160 * 1024) / lds;
  if (per_cu > 4) per_cu = 4;
  const int G = tile_workgroups(a.ntiles, MATCH_CUS * per_cu, max_workgroups);
  if (G > 0)
    hipLaunchKernelGGL(k_match_scan, dim3((unsigned)G), dim3(MATCH_BLOCK), (size_t)((S * L + 15) / 16 * 16), s, a);
  hipLaunchKernelGGL(k_match_join, dim3((unsigned)S), dim3(MATCH_BLOCK), 0, s, (const unsigned long long*)part, first, G, S);
  return hipGetLastError();
}

}  // namespace smx
