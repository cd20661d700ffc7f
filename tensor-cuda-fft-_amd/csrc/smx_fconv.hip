// smx_fconv.hip -- the per-bin channel contraction of the FFT convolutions (reference fft_tensor/optimized_ops.py:183-187
// and :247-251, `(x_freq.unsqueeze(1) * w_freq.unsqueeze(0)).sum(dim=2)`, which materialises a (B, Co, Ci, bins) product
// and reduces it): one small complex GEMM per frequency bin, channels innermost on every operand, complex64.
//
//   forward :  y[b, p, o]  = sum_i x[b, p, i] w[p, i, o]               x (B, P, Ci), w (P, Ci, Co), y (B, P, Co)
//   backward:  gx[b, p, i] = sum_o gy[b, p, o] conj(w[p, i, o])
//              gw[p, i, o] = sum_b conj(x[b, p, i]) gy[b, p, o]
//
// Three kernels of 256 threads, plain fp32 FMAs (four per complex product), every sum in ascending index order:
//
// k_bc_fwd.  A thread owns the output pair (o, o + 1) of one bin and BC_BT = 8 batch rows: 16 complex accumulators.  With
//   LB = the power of two at or above min(ceil(Co / 2), 256) lanes per bin a workgroup holds PT = 256 / LB bins.  Per chunk
//   of ICH = 2 LB input channels it stages x[b-tile, bins, chunk] in LDS as [bin][i][b] (a b-vector is 64 bytes: four
//   broadcast 16-byte reads), then walks i: one 16-byte load of w[p, i, o..o+1] where that address is 16-byte aligned, two
//   8-byte loads where it is not (an odd Co makes the rows alternate), 64 FMAs.  w is read once per batch tile; tiles are
//   numbered batch tile fastest, so the batch tiles of one bin run side by side and share w in L2.  More than 512 outputs:
//   the tile repeats per chunk of 512 (x is staged again).
// k_bc_gw.  The same thread map and the same LDS image of x; the thread holds gy[b-tile, p, o..o+1] in registers and per
//   input channel i sums conj(x) gy over b, then stores gw[p, i, o..o+1] (16 bytes where aligned).  More than 8 batch rows:
//   the SAME thread walks the batch tiles in order and, from the second on, starts each sum from the value it stored
//   itself before (a read-modify-write of its own elements: no atomics, the order is b = 0, 1, 2 ...).
// k_bc_gx.  The sum runs over w's contiguous axis, so w goes through LDS: a thread owns one input channel i of one bin
//   (LBI = power of two at or above min(Ci, 256) lanes per bin, PT = 256 / LBI bins) and 8 batch rows.  Per chunk of
//   OCH = min(8, 2 LBI) outputs the workgroup stages w[bins, i, chunk] as 256 rows of OCH + 1 elements (the odd pitch keeps
//   the 8-byte row reads of a wave on distinct banks) with 8-byte loads that are contiguous along o, and gy[b-tile, bins,
//   chunk] as [bin][o][b]; then 32 FMAs per staged element.  gx is written with 8-byte stores, contiguous along i.
//
// The arithmetic of an element never depends on which access width fetched it, so the results are a pure function of the
// inputs: row alignment does NOT enter (unlike smx_freq.h's rows).  No flag words, no atomics, no workgroup waits for
// another, nothing allocated, no host synchronisation.  A workgroup walks tiles blockIdx.x, + gridDim.x, ...: no unbounded
// size reaches a grid dimension, and max_workgroups caps the grid.
//
// The launchers and the size rule at the end of this file are declared in smx_kernels.h; the C entries are in smx_api.hip.
#include <cstdint>

#include "smx_kernels.h"

namespace smx {

constexpr int BC_BLOCK = 256;
constexpr int BC_BT = 8;                                   // batch rows per tile
constexpr int BC_SLOTS = 512;                              // b-vectors of the LDS image (32 KiB)
constexpr int BC_OCH = 8;                                  // outputs per chunk of k_bc_gx at most
constexpr int BC_WG = 8192;                                // workgroups at most (each walks its tiles)

namespace {

// acc += a b
__device__ __forceinline__ void cfma(float2& acc, float ax, float ay, float2 b) {
  acc.x = fmaf(ax, b.x, acc.x); acc.x = fmaf(-ay, b.y, acc.x);
  acc.y = fmaf(ax, b.y, acc.y); acc.y = fmaf(ay, b.x, acc.y);
}
// acc += conj(a) b
__device__ __forceinline__ void cfma_ca(float2& acc, float ax, float ay, float2 b) {
  acc.x = fmaf(ax, b.x, acc.x); acc.x = fmaf(ay, b.y, acc.x);
  acc.y = fmaf(ax, b.y, acc.y); acc.y = fmaf(-ay, b.x, acc.y);
}
// acc += a conj(b)
__device__ __forceinline__ void cfma_cb(float2& acc, float ax, float ay, float2 b) {
  acc.x = fmaf(ax, b.x, acc.x); acc.x = fmaf(ay, b.y, acc.x);
  acc.y = fmaf(ay, b.x, acc.y); acc.y = fmaf(-ax, b.y, acc.y);
}

// elements o, o + 1 of a row of n (o even, o < n): one 16-byte access where both exist and the address allows it
__device__ __forceinline__ void ld_pair(const float2* row, int o, int n, float2& a, float2& b) {
  const float2* q = row + o;
  if (o + 1 < n && ((uintptr_t)q & 15) == 0) {
    const float4 v = *reinterpret_cast<const float4*>(q);
    a = make_float2(v.x, v.y); b = make_float2(v.z, v.w);
  } else {
    a = q[0];
    b = o + 1 < n ? q[1] : make_float2(0.f, 0.f);
  }
}
__device__ __forceinline__ void st_pair(float2* row, int o, int n, float2 a, float2 b) {
  float2* q = row + o;
  if (o + 1 < n && ((uintptr_t)q & 15) == 0) {
    *reinterpret_cast<float4*>(q) = make_float4(a.x, a.y, b.x, b.y);
  } else {
    q[0] = a;
    if (o + 1 < n) q[1] = b;
  }
}

// xs[(q * ICH + ii) * 8 + b] = x[b0 + b, p0 + q, i0 + ii], zero outside B and P, for q < PT, ii < ni.  Lanes run along b:
// the LDS writes are contiguous, the global reads are eight rows of consecutive channels per wave.
__device__ __forceinline__ void stage_x(float2* xs, const float2* __restrict__ x, int B, long long P, int Ci, int b0,
                                        long long p0, int i0, int ni, int PT, int ICH) {
  const int total = PT * ni * BC_BT;
  for (int s = threadIdx.x; s < total; s += BC_BLOCK) {
    const int b = s & (BC_BT - 1), r = s >> 3;
    const int q = r / ni, ii = r - q * ni;
    float2 v = make_float2(0.f, 0.f);
    if (b0 + b < B && p0 + q < P) v = x[((long long)(b0 + b) * P + p0 + q) * Ci + i0 + ii];
    xs[(q * ICH + ii) * BC_BT + b] = v;
  }
}

}  // namespace

// lg: log2 LB.  np: tiles along P, nbt: along B, noc: chunks of 512 outputs (> 1 only with LB = 256).
__global__ __launch_bounds__(BC_BLOCK) void k_bc_fwd(const float2* __restrict__ x, const float2* __restrict__ w,
                                                     float2* __restrict__ y, int B, long long P, int Ci, int Co, int lg,
                                                     long long np, int nbt, int noc) {
  __shared__ __align__(16) float2 xs[BC_SLOTS * BC_BT];
  const int tid = threadIdx.x, LB = 1 << lg, PT = BC_BLOCK >> lg, ICH = BC_SLOTS / PT;
  const int pl = tid >> lg, j = tid & (LB - 1);
  const long long ntiles = np * nbt;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long p0 = (t / nbt) * PT, p = p0 + pl;
    const int b0 = (int)(t % nbt) * BC_BT;
    for (int oc = 0; oc < noc; ++oc) {
      const int o = 2 * (oc * LB + j);
      const bool act = p < P && o < Co;
      float2 a0[BC_BT], a1[BC_BT];
#pragma unroll
      for (int b = 0; b < BC_BT; ++b) a0[b] = a1[b] = make_float2(0.f, 0.f);
      for (int i0 = 0; i0 < Ci; i0 += ICH) {
        const int ni = Ci - i0 < ICH ? Ci - i0 : ICH;
        __syncthreads();                                  // the previous chunk's image has been read
        stage_x(xs, x, B, P, Ci, b0, p0, i0, ni, PT, ICH);
        __syncthreads();
        if (act) {
          const float2* wr = w + (p * Ci + i0) * (long long)Co;
          const float4* xv = reinterpret_cast<const float4*>(xs + (size_t)pl * ICH * BC_BT);
#pragma unroll 4
          for (int ii = 0; ii < ni; ++ii) {
            float2 wa, wb;
            ld_pair(wr + (long long)ii * Co, o, Co, wa, wb);
#pragma unroll
            for (int h = 0; h < BC_BT / 2; ++h) {
              const float4 v = xv[ii * (BC_BT / 2) + h];
              cfma(a0[2 * h], v.x, v.y, wa);     cfma(a1[2 * h], v.x, v.y, wb);
              cfma(a0[2 * h + 1], v.z, v.w, wa); cfma(a1[2 * h + 1], v.z, v.w, wb);
            }
          }
        }
      }
      if (act) {
#pragma unroll
        for (int b = 0; b < BC_BT; ++b)
          if (b0 + b < B) st_pair(y + ((long long)(b0 + b) * P + p) * Co, o, Co, a0[b], a1[b]);
      }
    }
  }
}

// The tiles are (tile along P, chunk of 512 outputs); the batch tiles are walked inside, in order.
__global__ __launch_bounds__(BC_BLOCK) void k_bc_gw(const float2* __restrict__ x, const float2* __restrict__ gy,
                                                    float2* __restrict__ gw, int B, long long P, int Ci, int Co, int lg,
                                                    long long np, int nbt, int noc) {
  __shared__ __align__(16) float2 xs[BC_SLOTS * BC_BT];
  const int tid = threadIdx.x, LB = 1 << lg, PT = BC_BLOCK >> lg, ICH = BC_SLOTS / PT;
  const int pl = tid >> lg, j = tid & (LB - 1);
  const long long ntiles = np * noc;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long p0 = (t / noc) * PT, p = p0 + pl;
    const int o = 2 * ((int)(t % noc) * LB + j);
    const bool act = p < P && o < Co;
    for (int bt = 0; bt < nbt; ++bt) {
      const int b0 = bt * BC_BT;
      float2 g0[BC_BT], g1[BC_BT];
#pragma unroll
      for (int b = 0; b < BC_BT; ++b) {
        g0[b] = g1[b] = make_float2(0.f, 0.f);
        if (act && b0 + b < B) ld_pair(gy + ((long long)(b0 + b) * P + p) * Co, o, Co, g0[b], g1[b]);
      }
      for (int i0 = 0; i0 < Ci; i0 += ICH) {
        const int ni = Ci - i0 < ICH ? Ci - i0 : ICH;
        __syncthreads();
        stage_x(xs, x, B, P, Ci, b0, p0, i0, ni, PT, ICH);
        __syncthreads();
        if (act) {
          float2* wr = gw + (p * Ci + i0) * (long long)Co;
          const float4* xv = reinterpret_cast<const float4*>(xs + (size_t)pl * ICH * BC_BT);
#pragma unroll 2
          for (int ii = 0; ii < ni; ++ii) {
            float2 s0 = make_float2(0.f, 0.f), s1 = make_float2(0.f, 0.f);
            if (bt > 0) ld_pair(wr + (long long)ii * Co, o, Co, s0, s1);      // what this thread stored for the rows before
#pragma unroll
            for (int h = 0; h < BC_BT / 2; ++h) {
              const float4 v = xv[ii * (BC_BT / 2) + h];
              cfma_ca(s0, v.x, v.y, g0[2 * h]);     cfma_ca(s1, v.x, v.y, g1[2 * h]);
              cfma_ca(s0, v.z, v.w, g0[2 * h + 1]); cfma_ca(s1, v.z, v.w, g1[2 * h + 1]);
            }
            st_pair(wr + (long long)ii * Co, o, Co, s0, s1);
          }
        }
      }
    }
  }
}

// lg: log2 LBI.  The tiles are (tile along P, chunk of 256 input channels, batch tile), batch tile fastest.
__global__ __launch_bounds__(BC_BLOCK) void k_bc_gx(const float2* __restrict__ gy, const float2* __restrict__ w,
                                                    float2* __restrict__ gx, int B, long long P, int Ci, int Co, int lg,
                                                    long long np, int nbt, int nic) {
  __shared__ __align__(16) float2 gs[BC_SLOTS * BC_BT];
  __shared__ float2 ws[BC_BLOCK * (BC_OCH + 1)];
  const int tid = threadIdx.x, LB = 1 << lg, PT = BC_BLOCK >> lg;
  const int OCH = 2 * LB < BC_OCH ? 2 * LB : BC_OCH;      // PT * OCH <= BC_SLOTS
  const int pl = tid >> lg, j = tid & (LB - 1);
  const long long per_p = (long long)nic * nbt, ntiles = np * per_p;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long p0 = (t / per_p) * PT, p = p0 + pl;
    const int rem = (int)(t % per_p), ic = rem / nbt, b0 = (rem % nbt) * BC_BT;
    const int i = ic * LB + j;
    const bool act = p < P && i < Ci;
    float2 acc[BC_BT];
#pragma unroll
    for (int b = 0; b < BC_BT; ++b) acc[b] = make_float2(0.f, 0.f);
    for (int o0 = 0; o0 < Co; o0 += OCH) {
      const int no = Co - o0 < OCH ? Co - o0 : OCH;
      __syncthreads();                                    // the previous chunk's images have been read
      for (int s = tid; s < BC_BLOCK * no; s += BC_BLOCK) {                 // w: row r of the workgroup = thread r's row
        const int r = s / no, oo = s - r * no;
        const long long pr = p0 + (r >> lg);
        const int ir = ic * LB + (r & (LB - 1));
        if (pr < P && ir < Ci) ws[r * (BC_OCH + 1) + oo] = w[(pr * Ci + ir) * (long long)Co + o0 + oo];
      }
      for (int s = tid; s < PT * no * BC_BT; s += BC_BLOCK) {
        const int b = s & (BC_BT - 1), r = s >> 3;
        const int q = r / no, oo = r - q * no;
        float2 v = make_float2(0.f, 0.f);
        if (b0 + b < B && p0 + q < P) v = gy[((long long)(b0 + b) * P + p0 + q) * Co + o0 + oo];
        gs[(q * OCH + oo) * BC_BT + b] = v;
      }
      __syncthreads();
      if (act) {
        const float4* gv = reinterpret_cast<const float4*>(gs + (size_t)pl * OCH * BC_BT);
        for (int oo = 0; oo < no; ++oo) {
          const float2 wv = ws[tid * (BC_OCH + 1) + oo];
#pragma unroll
          for (int h = 0; h < BC_BT / 2; ++h) {
            const float4 v = gv[oo * (BC_BT / 2) + h];
            cfma_cb(acc[2 * h], v.x, v.y, wv);
            cfma_cb(acc[2 * h + 1], v.z, v.w, wv);
          }
        }
      }
    }
    if (act) {
#pragma unroll
      for (int b = 0; b < BC_BT; ++b)
        if (b0 + b < B) gx[((long long)(b0 + b) * P + p) * Ci + i] = acc[b];
    }
  }
}

// every operand stays below 2^40 elements (the kernels index with 64 bits; the bound keeps the tile counts far from 2^63)
bool bin_contract_supported(int B, long long P, int Ci, int Co) {
  if (B < 1 || P < 1 || Ci < 1 || Co < 1 || P >= (1ll << 31)) return false;
  const long long lim = 1ll << 40;
  const long long c = Ci > Co ? Ci : Co;
  return (long long)Ci * Co < lim / P && (long long)B * c < lim / P;
}

namespace {

int lanes_log2(int n) {                                    // the power of two at or above min(n, 256)
  int lg = 0;
  while ((1 << lg) < n && lg < 8) ++lg;
  return lg;
}

}  // namespace

hipError_t launch_bin_contract_fwd(const float2* x, const float2* w, float2* y, int B, long long P, int Ci, int Co,
                                   int max_workgroups, hipStream_t s) {
  const int OP = (Co + 1) / 2, lg = lanes_log2(OP), PT = BC_BLOCK >> lg;
  const int noc = (OP + BC_BLOCK - 1) / BC_BLOCK, nbt = (B + BC_BT - 1) / BC_BT;
  const long long np = (P + PT - 1) / PT;
  const int G = tile_workgroups(np * nbt, BC_WG, max_workgroups);
  hipLaunchKernelGGL(k_bc_fwd, dim3((unsigned)G), dim3(BC_BLOCK), 0, s, x, w, y, B, P, Ci, Co, lg, np, nbt, noc);
  return hipGetLastError();
}

hipError_t launch_bin_contract_bwd(const float2* x, const float2* w, const float2* gy, float2* gx, float2* gw, int B,
                                   long long P, int Ci, int Co, int max_workgroups, hipStream_t s) {
  const int nbt = (B + BC_BT - 1) / BC_BT;
  if (gx) {
    const int lg = lanes_log2(Ci), PT = BC_BLOCK >> lg, nic = (Ci + BC_BLOCK - 1) / BC_BLOCK;
    const long long np = (P + PT - 1) / PT;
    const int G = tile_workgroups(np * nic * nbt, BC_WG, max_workgroups);
    hipLaunchKernelGGL(k_bc_gx, dim3((unsigned)G), dim3(BC_BLOCK), 0, s, gy, w, gx, B, P, Ci, Co, lg, np, nbt, nic);
  }
  if (gw) {
    const int OP = (Co + 1) / 2, lg = lanes_log2(OP), PT = BC_BLOCK >> lg, noc = (OP + BC_BLOCK - 1) / BC_BLOCK;
    const long long np = (P + PT - 1) / PT;
    const int G = tile_workgroups(np * noc, BC_WG, max_workgroups);
    hipLaunchKernelGGL(k_bc_gw, dim3((unsigned)G), dim3(BC_BLOCK), 0, s, x, gy, gw, B, P, Ci, Co, lg, np, nbt, noc);
  }
  return hipGetLastError();
}

}  // namespace smx
