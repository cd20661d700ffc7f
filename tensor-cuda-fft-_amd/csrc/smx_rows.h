// smx_rows.h -- per-row helpers of the one-wavefront-per-row kernels (smx_block.hip, smx_enh.hip):
// a row lives in one wavefront's registers, lane l holding elements (l + 64 c) VEC + [0, VEC), c < CH.
#pragma once
#include "smx_kernels.h"

namespace smx {

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

}  // namespace

}  // namespace smx
