// smx_rows.h -- the toolkit of the one-wavefront-per-row kernels (smx_block.hip, smx_enh.hip, and SpectralLayerNorm,
// the gate chain and the fusion line of smx_time.hip): a row lives in one wavefront's registers, lane l holding elements
// (l + 64 c) VEC + [0, VEC), c < CH.  Here: the wave sum, the Vec<VEC> chunk with its load policies, free functions on
// Vec<VEC>[CH] rows (load, store, LayerNorm statistics, the LayerNorm-backward step, the block partials of the parameter
// gradients), the dropout factors, and the host side: the (VEC, CH) dispatch on the row width and the launch of the
// kernels that walk rows ROW_WAVES at a time.
// 2-byte rows (IO = SMX_IO_BF16 / SMX_IO_F16): load_io / store_io move a chunk as 8 bytes per lane, widened
// exactly on load and rounded once at the store by widen2 / narrow2 of smx_launch.h -- the conversions of the
// streaming kernels, the fp16 guard against a multiply fused into the conversion included.  IO = 0 is load / store.
#pragma once
#include <type_traits>

#include "smx_launch.h"

namespace smx {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));      // (as smx_launch.h's, which only the device pass sees)

namespace {

// Sum over the 64 lanes, returned in every lane.  DPP row shifts + row broadcasts (six dependent
// VALU adds and one v_readlane) instead of six ds_bpermute round trips through the LDS crossbar.
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL,
                                                                ROW_MASK, 0xf, BOUND));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f<0x111, 0xf, true>(v);      // row_shr:1
  v += dpp_f<0x112, 0xf, true>(v);      // row_shr:2
  v += dpp_f<0x114, 0xf, true>(v);      // row_shr:4
  v += dpp_f<0x118, 0xf, true>(v);      // row_shr:8  -> lane 15 of each row holds the row sum
  v += dpp_f<0x142, 0xa, false>(v);     // row_bcast:15 into rows 1 and 3
  v += dpp_f<0x143, 0xc, false>(v);     // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// element of a row in memory: float, or the 16 bits of a bf16 / fp16
template <int IO> using io_elem = std::conditional_t<IO == 0, float, unsigned short>;

template <int VEC> struct Vec;
template <> struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
  }
  __device__ __forceinline__ void load_cached(const float* p) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(p);
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    f32x4 w; w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
    __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(p));
  }
};
template <> struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = __builtin_nontemporal_load(p); }
  __device__ __forceinline__ void load_cached(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { __builtin_nontemporal_store(v[0], p); }
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
template <> struct Vec<2> {
  float v[2];
  __device__ __forceinline__ void load(const float* p) {
    const f32x2 w = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p));
    v[0] = w.x; v[1] = w.y;
  }
  __device__ __forceinline__ void load_cached(const float* p) {
    const f32x2 w = *reinterpret_cast<const f32x2*>(p);
    v[0] = w.x; v[1] = w.y;
  }
  __device__ __forceinline__ void store(float* p) const {
    f32x2 w; w.x = v[0]; w.y = v[1];
    __builtin_nontemporal_store(w, reinterpret_cast<f32x2*>(p));
  }
};

// A chunk in the element type IO.  2-byte chunks exist for Vec<4> (8 bytes per lane); IO = 0 is load / store itself.
template <int IO, int VEC>
__device__ __forceinline__ void load_io(Vec<VEC>& r, const io_elem<IO>* p) {
  if constexpr (IO == 0) {
    r.load(p);
  } else {
    static_assert(VEC == 4, "2-byte rows move as Vec<4> chunks");
    const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    const unsigned w0 = w.x, w1 = w.y;      // (see load_rows, smx_launch.h)
    const cf a = widen2<IO>(w0), b = widen2<IO>(w1);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = b.x; r.v[3] = b.y;
  }
}
template <int IO, int VEC>
__device__ __forceinline__ void store_io(const Vec<VEC>& r, io_elem<IO>* p) {
  if constexpr (IO == 0) {
    r.store(p);
  } else {
    static_assert(VEC == 4, "2-byte rows move as Vec<4> chunks");
    u32x2 w;
    w.x = narrow2<IO>(r.v[0], r.v[1]); w.y = narrow2<IO>(r.v[2], r.v[3]);
    __builtin_nontemporal_store(w, reinterpret_cast<u32x2*>(p));
  }
}

template <int VEC, int CH>
__device__ __forceinline__ void zero(Vec<VEC> (&r)[CH]) {
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < VEC; ++i) r[c].v[i] = 0.f;
}

template <int VEC, int CH>
__device__ __forceinline__ void row_load(Vec<VEC> (&r)[CH], const float* p, int D, int lane) {
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (lane + 64 * c) * VEC;
    if (e < D) r[c].load(p + e);
    else
#pragma unroll
      for (int i = 0; i < VEC; ++i) r[c].v[i] = 0.f;
  }
}

// parameters (gamma / beta, rotation rows): re-read by every wavefront, so through the caches
template <int VEC, int CH>
__device__ __forceinline__ void row_load_cached(Vec<VEC> (&r)[CH], const float* p, int D, int lane, float dflt) {
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (lane + 64 * c) * VEC;
#pragma unroll
    for (int i = 0; i < VEC; ++i) r[c].v[i] = dflt;
    if (p && e < D) r[c].load_cached(p + e);
  }
}

template <int VEC, int CH>
__device__ __forceinline__ void row_store(const Vec<VEC> (&r)[CH], float* p, int D, int lane) {
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (lane + 64 * c) * VEC;
    if (e < D) r[c].store(p + e);
  }
}

template <int VEC, int CH>
__device__ __forceinline__ float row_sum(const Vec<VEC> (&r)[CH]) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < VEC; ++i) s += r[c].v[i];
  return s;
}

// sum of (r - mean)^2 over the D valid elements of this lane
template <int VEC, int CH>
__device__ __forceinline__ float row_sq(const Vec<VEC> (&r)[CH], float mean, int D, int lane) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (lane + 64 * c) * VEC;
    if (e < D)
#pragma unroll
      for (int i = 0; i < VEC; ++i) { const float d = r[c].v[i] - mean; s = fmaf(d, d, s); }
  }
  return s;
}

// (mean, rstd) of a D-wide row: biased variance, two passes over the registers (torch.nn.LayerNorm)
template <int VEC, int CH>
__device__ __forceinline__ cf row_stats(const Vec<VEC> (&r)[CH], int D, int lane, float eps) {
  const float inv_d = 1.f / (float)D;
  const float mean = wave_sum(row_sum(r)) * inv_d;
  const float var = wave_sum(row_sq(r, mean, D, lane)) * inv_d;
  return mk(mean, 1.f / sqrtf(var + eps));
}

// The LayerNorm-backward step of one row, in its two halves around the wave sums.  gh: gradient of the LayerNorm's
// output, xh: its normalised input (0 on the padding), u = gamma gh:
//   ln_bwd_acc, per element:  ag += gh xh,  ab += gh,  s1 += u,  s2 += u xh;  returns u
//   ln_bwd_apply, per row:    G += rstd (u - m1 - xh m2),  m1 = mean_d(u) = wave_sum(s1) / D,  m2 = mean_d(u xh)
__device__ __forceinline__ float ln_bwd_acc(float gh, float xh, float gm, float& ag, float& ab, float& s1, float& s2) {
  const float u = gm * gh;
  s1 += u;
  s2 = fmaf(u, xh, s2);
  ag = fmaf(gh, xh, ag);
  ab += gh;
  return u;
}
template <int VEC, int CH>
__device__ __forceinline__ void ln_bwd_apply(Vec<VEC> (&G)[CH], const Vec<VEC> (&u)[CH], const Vec<VEC> (&xh)[CH],
                                             float rstd, float m1, float m2) {
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < VEC; ++i) G[c].v[i] = fmaf(rstd, u[c].v[i] - m1 - xh[c].v[i] * m2, G[c].v[i]);
}

// mask * 1/(1-p) of elements e0 .. e0 + VEC - 1 of a batch row (e0 even): the pair (2i, 2i+1) shares one hash
template <int VEC>
__device__ __forceinline__ void drop_factors(float (&m)[VEC], unsigned key, unsigned long long e0, unsigned thr,
                                             float scale) {
#pragma unroll
  for (int i = 0; i < VEC; i += 2) {
    const unsigned h = drop_hash((unsigned)((e0 + i) >> 1), key);
    m[i] = (h & 0xffffu) >= thr ? scale : 0.f;
    m[i + 1] = (h >> 16) >= thr ? scale : 0.f;
  }
}

// Block partials of a LayerNorm's gamma / beta gradients: part[0][off + e] = sum_rows ag, part[1][off + e] = sum_rows
// ab, with part pointing at this block's (2, W) slab.  Waves are added in index order.
template <int VEC, int CH>
__device__ __forceinline__ void block_partials(const Vec<VEC> (&ag)[CH], const Vec<VEC> (&ab)[CH], float* part, int W,
                                               int off, int D, float (*red)[2][64 * VEC], int lane, int wv) {
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      red[wv][0][lane * VEC + i] = ag[c].v[i];
      red[wv][1][lane * VEC + i] = ab[c].v[i];
    }
    __syncthreads();
    if (wv == 0) {
      const int e = (lane + 64 * c) * VEC;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        if (e + i < D) {
          float a0 = 0.f, a1 = 0.f;
#pragma unroll
          for (int w2 = 0; w2 < ROW_WAVES; ++w2) {
            a0 += red[w2][0][lane * VEC + i];
            a1 += red[w2][1][lane * VEC + i];
          }
          part[off + e + i] = a0;
          part[W + off + e + i] = a1;
        }
      }
    }
    __syncthreads();
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// f(VEC, CH) as integral constants, CH the smallest of 1, STEP, STEP^2, ... <= MAX whose tile of 64 VEC CH elements
// covers a D-wide row; false (and no call) when none does.  A kernel family names its vector widths and ladders.
template <int VEC, int MAX, int STEP = 2, int CH = 1, typename Fn>
bool row_dispatch(int D, Fn&& f) {
  if constexpr (CH > MAX) {
    return false;
  } else {
    if (D > 64 * VEC * CH) return row_dispatch<VEC, MAX, STEP, CH * STEP>(D, f);
    f(std::integral_constant<int, VEC>(), std::integral_constant<int, CH>());
    return true;
  }
}

// Launch of a kernel that walks the rows ROW_WAVES at a time: its grid is what ln_num_blocks sizes the partial buffers by
template <typename... P, typename... A>
void row_launch(void (*k)(P...), long long rows, hipStream_t s, A... args) {
  hipLaunchKernelGGL(k, dim3(ln_num_blocks(rows)), dim3(64 * ROW_WAVES), 0, s, args...);
}

}  // namespace

}  // namespace smx
