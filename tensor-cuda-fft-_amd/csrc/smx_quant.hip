// smx_quant.hip -- the codecs of the compressed spectra: the polar quantiser (reference fft_tensor/polar_quantization.py
// :23-56, PolarQuantizer.quantize / dequantize) and the 8-bit logarithmic one (fft_tensor/zero_materialize.py:470-568,
// LogarithmicQuantizer.log8_encode / log8_decode / compress_sparse_freq / decompress_sparse_freq).  The reference runs each
// as a chain of whole-tensor passes (about fifteen for quantize); here every codec is ONE pass: 8 bytes read and 2 written
// per complex element on the way in, 2 read and 8 written on the way out, and the decoders look their at most 256 possible
// magnitudes / unit vectors up in LDS tables that each workgroup builds first, so no transcendental runs in their loops.
//
// Definitions (include/smx_quant.h states them for the caller).  With s = re^2 + im^2 (one product and one FMA, fp32) and
//   lg(z) = 0.5 log2(max(s, 1e-18))                      == log2(max(|z|, 1e-9)) for 1e-19 < |z| < 1e19
//   u = (lg - mag_min) * (Lm / (mag_max - mag_min + 1e-9)),   v = (atan2(im, re) + pi) * (Lp / 2 pi),   code = clamp(rint(.), 0, L)
// the range launch reduces the minimum and maximum of s itself (log2 is monotone: lg of the extreme s is the extreme lg)
// and applies lg once per end in the join, with the same device function that k_polar_quantize applies per element: an
// input whose s are all equal gets lg - mag_min == 0 exactly and all magnitude codes 0.
//
// Tiles on addresses.  The wide side (complex64 or fp32) is walked in GROUPS of four elements that start on a 16-byte
// address of that tensor: `head` elements (0 or 1 complex, 0..3 fp32) come before the first group and fewer than four after
// the last one; those are done one by one by the first threads of workgroup 0.  A lane moves a group as one or two 16-byte
// accesses on the wide side and FOUR bytes per code plane, so a wavefront reads / writes 256 contiguous bytes of a plane.
// A plane may start at any byte: where (plane + head) is 4-byte aligned the four codes are one dword access, elsewhere four
// byte accesses (the same bytes; uniform over the launch).  Workgroup g of G walks groups g*256+tid, +G*256, ...
// Only vector stores and plain C++.  No atomics on memory, no flag words, no workgroup waits for another: every result is a
// pure function of the inputs (codes do not depend on the alignment either: a head element runs the same arithmetic).
//
// The launchers at the end of this file are declared in smx_kernels.h (weak there); the C entries are in smx_api.hip.
#include <cstdint>

#include "smx_kernels.h"

namespace smx {

constexpr int QUANT_BLOCK = 256;
constexpr int QUANT_CUS = 256, QUANT_MAX_WG = 8 * QUANT_CUS;       // 8 workgroups of 256 threads per CU stay resident
constexpr float QUANT_PI = 3.14159265358979323846f;

struct QuantArgs {
  const void* in0;                  // wide side or first plane
  const void* in1;                  // second plane (decoders)
  void* out0;
  void* out1;
  long long n, ngroups;
  int head;                         // elements before the first group
  int al0, al1;                     // plane 0 / 1: (plane + head) is 4-byte aligned
  float f0, f1, f2, f3;             // polar: mag_min, magnitude scale / span, phase scale; see the kernels
  float L0, L1;                     // top codes Lm, Lp
};

// ---- element arithmetic ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float polar_s(float re, float im) { return __builtin_fmaf(re, re, im * im); }
__device__ __forceinline__ float polar_lg(float s) { return 0.5f * log2f(fmaxf(s, 1e-18f)); }
__device__ __forceinline__ unsigned code_rint(float t, float top) {      // clamp(rint(t), 0, top); a NaN gives 0
  return (unsigned)fminf(fmaxf(rintf(t), 0.f), top);
}
__device__ __forceinline__ unsigned polar_mag_code(float re, float im, const QuantArgs& a) {
  return code_rint((polar_lg(polar_s(re, im)) - a.f0) * a.f1, a.L0);
}
__device__ __forceinline__ unsigned polar_phase_code(float re, float im, const QuantArgs& a) {
  return code_rint((atan2f(im, re) + QUANT_PI) * a.f2, a.L1);
}
__device__ __forceinline__ unsigned log8_code(float x) {
  const float t = (log2f(fabsf(x) + 1e-8f) + 8.f) * 0.0625f * 127.f;     // (lg + 8) / 16 * 127: the division is exact
  const unsigned q = (unsigned)fminf(fmaxf(t, 0.f), 127.f);              // truncation; a NaN gives 0
  return (x >= 0.f ? 128u : 0u) | q;
}

// ---- four codes of a plane ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void st_codes(unsigned char* p, unsigned w, int aligned) {
  if (aligned) {
    *reinterpret_cast<unsigned*>(p) = w;
  } else {
    p[0] = (unsigned char)w; p[1] = (unsigned char)(w >> 8); p[2] = (unsigned char)(w >> 16); p[3] = (unsigned char)(w >> 24);
  }
}
__device__ __forceinline__ unsigned ld_codes(const unsigned char* p, int aligned) {
  if (aligned) return *reinterpret_cast<const unsigned*>(p);
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}

// The walk every streaming kernel runs: group(i) moves the four elements from i on, one(i) element i.
template <class Group, class One>
__device__ __forceinline__ void quant_walk(const QuantArgs& a, Group group, One one) {
  const long long step = (long long)gridDim.x * QUANT_BLOCK;
  for (long long g = (long long)blockIdx.x * QUANT_BLOCK + threadIdx.x; g < a.ngroups; g += step) group(a.head + 4 * g);
  if (blockIdx.x == 0) {
    const long long tail = a.head + 4 * a.ngroups, t = threadIdx.x;
    if (t < a.head) one(t);
    else if (tail + (t - a.head) < a.n) one(tail + (t - a.head));
  }
}

// ---- polar: range ------------------------------------------------------------------------------------------------------------
// part[g] = (min, max) of s over the elements workgroup g walks; every workgroup of the grid writes its pair (a workgroup
// without elements writes (+inf, -inf)).
__global__ __launch_bounds__(QUANT_BLOCK) void k_polar_range(QuantArgs a) {
  __shared__ float rmin[QUANT_BLOCK], rmax[QUANT_BLOCK];
  const float* z = static_cast<const float*>(a.in0);
  float lo = __builtin_inff(), hi = -__builtin_inff();
  quant_walk(a,
    [&](long long i) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(z + 2 * i), q = *reinterpret_cast<const f32x4*>(z + 2 * i + 4);
      const float s0 = polar_s(p.x, p.y), s1 = polar_s(p.z, p.w), s2 = polar_s(q.x, q.y), s3 = polar_s(q.z, q.w);
      lo = fminf(fminf(lo, fminf(s0, s1)), fminf(s2, s3));
      hi = fmaxf(fmaxf(hi, fmaxf(s0, s1)), fmaxf(s2, s3));
    },
    [&](long long i) {
      const float s = polar_s(z[2 * i], z[2 * i + 1]);
      lo = fminf(lo, s); hi = fmaxf(hi, s);
    });
  const int tid = threadIdx.x;
  rmin[tid] = lo; rmax[tid] = hi;
  __syncthreads();
  for (int d = QUANT_BLOCK / 2; d > 0; d >>= 1) {
    if (tid < d) { rmin[tid] = fminf(rmin[tid], rmin[tid + d]); rmax[tid] = fmaxf(rmax[tid], rmax[tid + d]); }
    __syncthreads();
  }
  if (tid == 0) static_cast<float2*>(a.out0)[blockIdx.x] = make_float2(rmin[0], rmax[0]);
}

// out2 = (lg(min over the G pairs), lg(max over them)).  One workgroup.
__global__ __launch_bounds__(QUANT_BLOCK) void k_polar_range_join(const float2* __restrict__ part, float* __restrict__ out2,
                                                                 int G) {
  __shared__ float rmin[QUANT_BLOCK], rmax[QUANT_BLOCK];
  const int tid = threadIdx.x;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int g = tid; g < G; g += QUANT_BLOCK) { const float2 v = part[g]; lo = fminf(lo, v.x); hi = fmaxf(hi, v.y); }
  rmin[tid] = lo; rmax[tid] = hi;
  __syncthreads();
  for (int d = QUANT_BLOCK / 2; d > 0; d >>= 1) {
    if (tid < d) { rmin[tid] = fminf(rmin[tid], rmin[tid + d]); rmax[tid] = fmaxf(rmax[tid], rmax[tid + d]); }
    __syncthreads();
  }
  if (tid == 0) { out2[0] = polar_lg(rmin[0]); out2[1] = polar_lg(rmax[0]); }
}

// ---- polar: quantize ---------------------------------------------------------------------------------------------------------
// f0 = mag_min, f1 = Lm / (mag_max - mag_min + 1e-9), f2 = Lp / 2 pi, L0 = Lm, L1 = Lp
__global__ __launch_bounds__(QUANT_BLOCK) void k_polar_quantize(QuantArgs a) {
  const float* z = static_cast<const float*>(a.in0);
  unsigned char* mq = static_cast<unsigned char*>(a.out0);
  unsigned char* pq = static_cast<unsigned char*>(a.out1);
  quant_walk(a,
    [&](long long i) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(z + 2 * i), q = *reinterpret_cast<const f32x4*>(z + 2 * i + 4);
      const unsigned m = polar_mag_code(p.x, p.y, a) | (polar_mag_code(p.z, p.w, a) << 8)
                         | (polar_mag_code(q.x, q.y, a) << 16) | (polar_mag_code(q.z, q.w, a) << 24);
      const unsigned ph = polar_phase_code(p.x, p.y, a) | (polar_phase_code(p.z, p.w, a) << 8)
                          | (polar_phase_code(q.x, q.y, a) << 16) | (polar_phase_code(q.z, q.w, a) << 24);
      st_codes(mq + i, m, a.al0);
      st_codes(pq + i, ph, a.al1);
    },
    [&](long long i) {
      const float re = z[2 * i], im = z[2 * i + 1];
      mq[i] = (unsigned char)polar_mag_code(re, im, a);
      pq[i] = (unsigned char)polar_phase_code(re, im, a);
    });
}

// ---- polar: dequantize -------------------------------------------------------------------------------------------------------
// f0 = mag_min, f1 = mag_max - mag_min, L0 = Lm, L1 = Lp.  The tables hold all 256 byte values (a code above the top one
// extrapolates, as the reference's arithmetic does), so no code indexes outside them.
__global__ __launch_bounds__(QUANT_BLOCK) void k_polar_dequantize(QuantArgs a) {
  __shared__ float tmag[256];
  __shared__ float2 tdir[256];
  {
    const int c = threadIdx.x;                                           // QUANT_BLOCK == 256: an entry of each per thread
    tmag[c] = exp2f((float)c / a.L0 * a.f1 + a.f0);
    float sn, cs;
    sincospif(2.f * ((float)c / a.L1) - 1.f, &sn, &cs);                  // (cos, sin)(c / Lp 2 pi - pi), reduced exactly
    tdir[c] = make_float2(cs, sn);
  }
  __syncthreads();
  const unsigned char* mq = static_cast<const unsigned char*>(a.in0);
  const unsigned char* pq = static_cast<const unsigned char*>(a.in1);
  float* z = static_cast<float*>(a.out0);
  quant_walk(a,
    [&](long long i) {
      const unsigned m = ld_codes(mq + i, a.al0), ph = ld_codes(pq + i, a.al1);
      const float m0 = tmag[m & 255u], m1 = tmag[(m >> 8) & 255u], m2 = tmag[(m >> 16) & 255u], m3 = tmag[m >> 24];
      const float2 d0 = tdir[ph & 255u], d1 = tdir[(ph >> 8) & 255u], d2 = tdir[(ph >> 16) & 255u], d3 = tdir[ph >> 24];
      f32x4 p, q;
      p.x = m0 * d0.x; p.y = m0 * d0.y; p.z = m1 * d1.x; p.w = m1 * d1.y;
      q.x = m2 * d2.x; q.y = m2 * d2.y; q.z = m3 * d3.x; q.w = m3 * d3.y;
      *reinterpret_cast<f32x4*>(z + 2 * i) = p;
      *reinterpret_cast<f32x4*>(z + 2 * i + 4) = q;
    },
    [&](long long i) {
      const float m = tmag[mq[i]];
      const float2 d = tdir[pq[i]];
      z[2 * i] = m * d.x; z[2 * i + 1] = m * d.y;
    });
}

// ---- log8 --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QUANT_BLOCK) void k_log8_encode(QuantArgs a) {
  const float* x = static_cast<const float*>(a.in0);
  unsigned char* e = static_cast<unsigned char*>(a.out0);
  quant_walk(a,
    [&](long long i) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(x + i);
      st_codes(e + i, log8_code(p.x) | (log8_code(p.y) << 8) | (log8_code(p.z) << 16) | (log8_code(p.w) << 24), a.al0);
    },
    [&](long long i) { e[i] = (unsigned char)log8_code(x[i]); });
}

// the 256 values a log8 byte decodes to: sign (bit 7 set: +) times 2^(q / 127 * 16 - 8)
__device__ __forceinline__ void log8_table(float* t) {
  const int c = threadIdx.x;
  const float m = exp2f((float)(c & 127) / 127.f * 16.f - 8.f);
  t[c] = (c & 128) ? m : -m;
}

__global__ __launch_bounds__(QUANT_BLOCK) void k_log8_decode(QuantArgs a) {
  __shared__ float tab[256];
  log8_table(tab);
  __syncthreads();
  const unsigned char* e = static_cast<const unsigned char*>(a.in0);
  float* x = static_cast<float*>(a.out0);
  quant_walk(a,
    [&](long long i) {
      const unsigned w = ld_codes(e + i, a.al0);
      f32x4 p;
      p.x = tab[w & 255u]; p.y = tab[(w >> 8) & 255u]; p.z = tab[(w >> 16) & 255u]; p.w = tab[w >> 24];
      *reinterpret_cast<f32x4*>(x + i) = p;
    },
    [&](long long i) { x[i] = tab[e[i]]; });
}

// the codec on both parts of an interleaved complex64 tensor
__global__ __launch_bounds__(QUANT_BLOCK) void k_log8_encode_c64(QuantArgs a) {
  const float* z = static_cast<const float*>(a.in0);
  unsigned char* rq = static_cast<unsigned char*>(a.out0);
  unsigned char* iq = static_cast<unsigned char*>(a.out1);
  quant_walk(a,
    [&](long long i) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(z + 2 * i), q = *reinterpret_cast<const f32x4*>(z + 2 * i + 4);
      st_codes(rq + i, log8_code(p.x) | (log8_code(p.z) << 8) | (log8_code(q.x) << 16) | (log8_code(q.z) << 24), a.al0);
      st_codes(iq + i, log8_code(p.y) | (log8_code(p.w) << 8) | (log8_code(q.y) << 16) | (log8_code(q.w) << 24), a.al1);
    },
    [&](long long i) {
      rq[i] = (unsigned char)log8_code(z[2 * i]);
      iq[i] = (unsigned char)log8_code(z[2 * i + 1]);
    });
}

__global__ __launch_bounds__(QUANT_BLOCK) void k_log8_decode_c64(QuantArgs a) {
  __shared__ float tab[256];
  log8_table(tab);
  __syncthreads();
  const unsigned char* rq = static_cast<const unsigned char*>(a.in0);
  const unsigned char* iq = static_cast<const unsigned char*>(a.in1);
  float* z = static_cast<float*>(a.out0);
  quant_walk(a,
    [&](long long i) {
      const unsigned r = ld_codes(rq + i, a.al0), m = ld_codes(iq + i, a.al1);
      f32x4 p, q;
      p.x = tab[r & 255u]; p.y = tab[m & 255u]; p.z = tab[(r >> 8) & 255u]; p.w = tab[(m >> 8) & 255u];
      q.x = tab[(r >> 16) & 255u]; q.y = tab[(m >> 16) & 255u]; q.z = tab[r >> 24]; q.w = tab[m >> 24];
      *reinterpret_cast<f32x4*>(z + 2 * i) = p;
      *reinterpret_cast<f32x4*>(z + 2 * i + 4) = q;
    },
    [&](long long i) { z[2 * i] = tab[rq[i]]; z[2 * i + 1] = tab[iq[i]]; });
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
size_t quant_range_part_bytes() { return al((size_t)QUANT_MAX_WG * sizeof(float2)); }

// n > 0.  wide: the 16-byte-walked tensor, `esize` bytes per element (8 complex64, 4 fp32); p0 / p1: the code planes.
static int quant_setup(QuantArgs& a, const void* wide, int esize, const void* p0, const void* p1, long long n,
                       int max_workgroups) {
  const int mis = (int)((uintptr_t)wide & 15);
  long long head = mis ? (16 - mis) / esize : 0;
  if (head > n) head = n;
  a.n = n; a.head = (int)head; a.ngroups = (n - head) / 4;
  a.al0 = (((uintptr_t)p0 + (uintptr_t)head) & 3) == 0;
  a.al1 = (((uintptr_t)p1 + (uintptr_t)head) & 3) == 0;
  const int G = tile_workgroups((a.ngroups + QUANT_BLOCK - 1) / QUANT_BLOCK, QUANT_MAX_WG, max_workgroups);
  return G > 0 ? G : 1;                                                   // head and tail alone still need workgroup 0
}

hipError_t launch_polar_range(const float2* z, long long n, float* out2, float2* part, int max_workgroups, hipStream_t s) {
  QuantArgs a{};
  const int G = quant_setup(a, z, 8, nullptr, nullptr, n, max_workgroups);
  a.in0 = z; a.out0 = part;
  hipLaunchKernelGGL(k_polar_range, dim3((unsigned)G), dim3(QUANT_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_polar_range_join, dim3(1), dim3(QUANT_BLOCK), 0, s, (const float2*)part, out2, G);
  return hipGetLastError();
}

hipError_t launch_polar_quantize(const float2* z, unsigned char* mag_q, unsigned char* phase_q, long long n, int mag_bits,
                                 int phase_bits, float mag_min, float mag_max, int max_workgroups, hipStream_t s) {
  QuantArgs a{};
  const int G = quant_setup(a, z, 8, mag_q, phase_q, n, max_workgroups);
  a.in0 = z; a.out0 = mag_q; a.out1 = phase_q;
  a.L0 = (float)((1 << mag_bits) - 1); a.L1 = (float)((1 << phase_bits) - 1);
  a.f0 = mag_min;
  a.f1 = (float)((double)a.L0 / ((double)mag_max - (double)mag_min + 1e-9));
  a.f2 = (float)((double)a.L1 / (2.0 * 3.14159265358979323846));
  hipLaunchKernelGGL(k_polar_quantize, dim3((unsigned)G), dim3(QUANT_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_polar_dequantize(const unsigned char* mag_q, const unsigned char* phase_q, float2* z, long long n,
                                   int mag_bits, int phase_bits, float mag_min, float mag_max, int max_workgroups,
                                   hipStream_t s) {
  QuantArgs a{};
  const int G = quant_setup(a, z, 8, mag_q, phase_q, n, max_workgroups);
  a.in0 = mag_q; a.in1 = phase_q; a.out0 = z;
  a.L0 = (float)((1 << mag_bits) - 1); a.L1 = (float)((1 << phase_bits) - 1);
  a.f0 = mag_min;
  a.f1 = (float)((double)mag_max - (double)mag_min);
  hipLaunchKernelGGL(k_polar_dequantize, dim3((unsigned)G), dim3(QUANT_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_log8_encode(const float* x, unsigned char* e, long long n, int max_workgroups, hipStream_t s) {
  QuantArgs a{};
  const int G = quant_setup(a, x, 4, e, nullptr, n, max_workgroups);
  a.in0 = x; a.out0 = e;
  hipLaunchKernelGGL(k_log8_encode, dim3((unsigned)G), dim3(QUANT_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_log8_decode(const unsigned char* e, float* x, long long n, int max_workgroups, hipStream_t s) {
  QuantArgs a{};
  const int G = quant_setup(a, x, 4, e, nullptr, n, max_workgroups);
  a.in0 = e; a.out0 = x;
  hipLaunchKernelGGL(k_log8_decode, dim3((unsigned)G), dim3(QUANT_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_log8_encode_c64(const float2* z, unsigned char* re_q, unsigned char* im_q, long long n, int max_workgroups,
                                  hipStream_t s) {
  QuantArgs a{};
  const int G = quant_setup(a, z, 8, re_q, im_q, n, max_workgroups);
  a.in0 = z; a.out0 = re_q; a.out1 = im_q;
  hipLaunchKernelGGL(k_log8_encode_c64, dim3((unsigned)G), dim3(QUANT_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_log8_decode_c64(const unsigned char* re_q, const unsigned char* im_q, float2* z, long long n,
                                  int max_workgroups, hipStream_t s) {
  QuantArgs a{};
  const int G = quant_setup(a, z, 8, re_q, im_q, n, max_workgroups);
  a.in0 = re_q; a.in1 = im_q; a.out0 = z;
  hipLaunchKernelGGL(k_log8_decode_c64, dim3((unsigned)G), dim3(QUANT_BLOCK), 0, s, a);
  return hipGetLastError();
}

}  // namespace smx
