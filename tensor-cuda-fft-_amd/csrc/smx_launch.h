// smx_launch.h -- pieces shared by the kernel translation units (smx_decim.hip, smx_fourstep.hip):
// the LDS declaration, the workgroup -> work item map and the launch-in-rounds helper.
#pragma once
#include <type_traits>
#ifdef SMX_LAUNCH_TRACE
#include <typeinfo>
#endif
#include "smx_kernels.h"

namespace smx {

// One LDS array only (guide: a second __shared__ object can de-pipeline the loop).
// 2 x 32 KiB exchange buffers; 2 workgroups per CU fit in the 160 KiB LDS.
// (the unpack exchange publishes at most 32 slots per thread per round = the same 64 KiB)
// (+ 2 KiB so that the staged filter tile of the NB == 1 kernels, WL_ELEMS, fits behind the first buffer)
#define SMX_LDS_DECL __shared__ cf lds[EX + WL_ELEMS]
static_assert(WL_ELEMS >= EX, "the second exchange buffer lives in the same space");

// ---- workgroup -> (batch row, d-tile, residue chunk, residue rotation) ---------------------------
// Blocks are dealt round-robin over the 8 XCDs (bid % 8), each with its own L2.  Within one tile
// every row a workgroup touches has the same address bits [7..13] (at D = 256: d-tile -> bits 7-9,
// residue -> bits 10-13), so the naive b-major order makes all workgroups of an XCD hit the same L2 channel
// slot at the same time.  map == 2 hands each XCD all d-tiles and a spread of residue phases (all 64
// (d-tile pair, residue) combinations once per 64 workgroups) and batch rows 8 apart: measured
// +11 % read and +15 % write bandwidth on the same access pattern (tools/probe_stride.hip).
// Placement only affects speed: every mapping is a bijection onto the same work items.
struct WgItem { int b, dt, c, rot; };
__device__ __forceinline__ WgItem wg_map(int bid, int B, int ndt, int nsplit, int lc, int map) {
  WgItem w;
  const int per = B * nsplit;                 // (b, c) pairs per d-tile
  // map == 3 | a << 8 | b << 16: rotation lattice rot = (a l2 + b dt) mod lc, for tools/rot_scan.py
  const int ra = (map >> 8) & 0xff, rb = (map >> 16) & 0xff;
  map &= 0xff;
  if ((map == 2 || map == 3) && per % 8 == 0 && (B % 8 == 0 || B == 1 || 8 % B == 0)) {
    const int x = bid & 7, l = bid >> 3;
    w.dt = l % ndt;
    const int l2 = l / ndt;                   // 0 .. per/8 - 1
    if (B % 8 == 0) { const int g = B / 8; w.b = x + 8 * (l2 % g); w.c = l2 / g; }
    else { const int g = 8 / B; w.b = x % B; w.c = (x / B) + g * l2; }      // B in {1,2,4}: XCDs share rows
    w.rot = map == 3 ? (l2 * ra + w.dt * rb) % lc : (l2 + (lc >> 1) * (w.dt & 1)) % lc;
    return w;
  }
  w.c = bid % nsplit;
  const int wg = bid / nsplit;
  w.b = wg / ndt; w.dt = wg % ndt;
  w.rot = map == 1 ? (int)(((unsigned)bid * 7u) % (unsigned)lc) : 0;
  return w;
}

// ---- the streamed tensors as raw buffers (round 4) -----------------------------------------------
// One batch row of x / y / g / grad_x is described to the hardware as a raw buffer (base + byte count), and a tile
// access is buffer_load / buffer_store_dwordx2 with ONE per-thread 32-bit offset (row t L + r, this thread's channel
// pair) and the row pitch of the thread's 16 rows, u 16 L D 4 bytes, as the instruction's SCALAR offset.  Against
// global_load with a 64-bit address per row this removes 16 v_lshl_add_u64 + the 64-bit row arithmetic per tile
// (about 30 of the loop's 530 vector instructions in round 3), halves the SGPRs the row pitches occupy, and states
// the streaming policy in the instruction itself: round 3's __builtin_nontemporal_store lost its hint on 12 of the
// 16 stores of a tile somewhere in the optimiser (llvm-objdump of the shipped kernel: 4 x `nt`, 12 x plain).
// Zero-padded rows (PAD: x / y hold R < N rows): the row pitch moves into the per-thread offset, and the buffer's
// range check (offset >= R D 4 bytes: loads return 0, stores are dropped) is the predicate.
// Needs R D 4 < 2^31 (make_plan sends larger batch rows to the direct plan; R D 2 for 2-byte tensors, IO below).
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
constexpr int BUF_NT = 2;          // cache policy operand of the buffer intrinsics: slc = `nt` on gfx950
// IO = element type of the streamed tensor (SMX_IO_*): 0 f32 -- a channel pair is buffer_load / buffer_store_dwordx2;
// 1 bf16, 2 fp16 -- the same tile walk with the packed channel pair in ONE dword (buffer_load / buffer_store_dword),
// every pitch and the range in 2-byte elements.  ES = bytes per element.
template <int IO>
struct RowBufT {
  static constexpr unsigned ES = IO == 0 ? 4u : 2u;
  __amdgpu_buffer_rsrc_t rs;       // batch row b: base + b R D elements, R D ES bytes
  unsigned vo;                     // (t L D + d) ES: this thread's channel pair in row t L
  unsigned su;                     // 16 L D ES: bytes between a thread's consecutive rows
  unsigned rowb;                   // D ES
};
using RowBuf = RowBufT<0>;
// row0 = the batch row, base + b R D elements (f32: the caller forms it, see below).
// in_range = false (a lane whose channel pair lies past D): every offset the lane forms is 2^31 + (an offset inside
// the batch row) -- in [2^31, 2^32), past any buffer and short of wrapping: its stores are dropped and its loads
// return 0 without a branch around the tile code
template <int IO = 0>
__device__ __forceinline__ RowBufT<IO> row_buf(const void* row0, const Geom& g, int t, int d, bool in_range = true) {
  constexpr unsigned ES = RowBufT<IO>::ES;
  RowBufT<IO> rb;
  rb.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(row0), 0, (int)((unsigned)g.R * (unsigned)g.D * ES),
                                            0x00020000);
  rb.rowb = (unsigned)g.D * ES;
  rb.vo = in_range ? ((unsigned)t * (unsigned)g.L * (unsigned)g.D + (unsigned)d) * ES : 0x80000000u;
  rb.su = 16u * (unsigned)g.L * rb.rowb;                 // (uniform: it is the instructions' scalar offset)
  return rb;
}
// The same from the tensor base and b, for the 2-byte kernels.  Two spellings on purpose: WHERE base + b R D is formed
// (in the caller's argument list, or in here behind the other arguments) decides the instruction order of the
// kernels' scalar prologue, and so does a call from one of these bodies into the other.  The f32
// kernels have always formed it in the call, the 2-byte kernels in here; each keeps its spelling so that each kernel
// keeps its machine code.  Change both bodies together.
template <int IO>
__device__ __forceinline__ RowBufT<IO> row_buf(const void* base, int b, const Geom& g, int t, int d,
                                               bool in_range = true) {
  constexpr unsigned ES = RowBufT<IO>::ES;
  RowBufT<IO> rb;
  char* row0 = const_cast<char*>(static_cast<const char*>(base)) + (size_t)b * g.R * g.D * ES;
  rb.rs = __builtin_amdgcn_make_buffer_rsrc(row0, 0, (int)((unsigned)g.R * (unsigned)g.D * ES), 0x00020000);
  rb.rowb = (unsigned)g.D * ES;
  rb.vo = in_range ? ((unsigned)t * (unsigned)g.L * (unsigned)g.D + (unsigned)d) * ES : 0x80000000u;
  rb.su = 16u * (unsigned)g.L * rb.rowb;
  return rb;
}
// 2-byte elements: loads widen exactly (bf16: the high half of an f32; fp16: v_cvt_f32_f16), stores round once, to
// nearest even: bf16 by the plain cast (v_cvt_pk_bf16_f32 -- a NaN stays a NaN), fp16 by the IEEE conversion
// (v_cvt_f16_f32: overflow to +-inf; never the round-toward-zero v_cvt_pkrtz) -- the results of
// torch.Tensor.to(dtype) on the f32 values, bit for bit.
template <int IO>
__device__ __forceinline__ cf widen2(unsigned w) {
  if constexpr (IO == 1) {
    return mk(__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u));
  } else {
    const f16x2_t h = __builtin_bit_cast(f16x2_t, w);
    return mk((float)h.x, (float)h.y);
  }
}
template <int IO>
__device__ __forceinline__ unsigned narrow2(float fx, float fy) {
  if constexpr (IO == 1) {
    bf16x2_t h;
    h.x = (__bf16)fx; h.y = (__bf16)fy;
    return __builtin_bit_cast(unsigned, h);
  } else {
    // the f32 values first: left to itself the compiler folds a preceding multiply (the dropout scale) into the
    // conversion (v_fma_mixlo_f16 -- one rounding instead of the f32 path's two: measured 80 of 0.5 M elements off)
    asm("" : "+v"(fx));
    asm("" : "+v"(fy));
    f16x2_t h;
    h.x = (_Float16)fx; h.y = (_Float16)fy;
    return __builtin_bit_cast(unsigned, h);
  }
}
// rows u = U0 .. U0+CNT-1 of tile r: row (t + 16 u) L + r
template <int U0, int CNT, bool PAD, int IO>
__device__ __forceinline__ void load_rows(const RowBufT<IO>& rb, int r, cf (&v)[16]) {
  const unsigned vr = rb.vo + (unsigned)r * rb.rowb;
#pragma unroll
  for (int u = U0; u < U0 + CNT; ++u) {
    const unsigned vo = PAD ? vr + (unsigned)u * rb.su : vr, so = PAD ? 0u : (unsigned)u * rb.su;
    float fx, fy;
    if constexpr (IO == 0) {
      const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rb.rs, vo, so, BUF_NT);
      const unsigned wx = w.x, wy = w.y;      // (bit_cast straight from a vector ELEMENT reads element 0 twice: clang 22)
      fx = __builtin_bit_cast(float, wx); fy = __builtin_bit_cast(float, wy);
    } else {
      const cf e = widen2<IO>(__builtin_amdgcn_raw_buffer_load_b32(rb.rs, vo, so, BUF_NT));
      fx = e.x; fy = e.y;
    }
    // two scalars from here on: left as <2 x float> the optimiser turns the first butterflies into v_pk_add_f32,
    // which issue at half the rate of the scalar adds with two waves per SIMD (tools/probe_valu.hip, round 3)
    asm("" : "+v"(fx));
    asm("" : "+v"(fy));
    v[u] = mk(fx, fy);
  }
}
// mask (wave-uniform, 16 bits; st_mask() below): row u goes out with the default write-back policy iff bit u is set, the
// others with the streaming hint.  DecimArgs::st_plain of the 16 bits are set (0, 1, 2 or 4, chosen from the output's
// bytes in smx_api decim_args); which ones is the store layout (store_layout(), smx_kernels.h).  About 64 MiB of an
// output tensor written back through L2 / Infinity Cache costs nothing (it drains under the next launch's reads); all
// 16 rows streaming were 9 % slower per C2 step, all 16 cached 13 % (profiles/r04_store_policy.txt).  The policy is an
// immediate of the store, so every row is two store forms behind a scalar branch: sixteen s_bitcmp1 + branch per tile,
// nothing per lane.
__device__ __forceinline__ unsigned rot16(unsigned m, unsigned s) {
  s &= 15u;
  return ((m >> s) | (m << (16u - s))) & 0xffffu;
}
// sw = (wave of the workgroup) >> a.st_wsh, a scalar the caller forms once per launch (readfirstlane: the compiler
// does not know that t >> 2 is wave-uniform, and a per-lane mask would turn the branches into exec masks)
__device__ __forceinline__ unsigned st_tile_mask(const DecimArgs& a, int r, int sw) {
  return rot16(a.st_mask, (unsigned)((r >> a.st_rsh) + sw));
}
template <bool PAD, int IO>
__device__ __forceinline__ void store_rows(const RowBufT<IO>& rb, int r, const cf (&v)[16], unsigned mask) {
  const unsigned vr = rb.vo + (unsigned)r * rb.rowb;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const float fx = v[u].x, fy = v[u].y;
    std::conditional_t<IO == 0, u32x2, unsigned> w;
    if constexpr (IO == 0) { w.x = __builtin_bit_cast(unsigned, fx); w.y = __builtin_bit_cast(unsigned, fy); }
    else w = narrow2<IO>(fx, fy);
    const unsigned vo = PAD ? vr + (unsigned)u * rb.su : vr, so = PAD ? 0u : (unsigned)u * rb.su;
    if constexpr (IO == 0) {
      if (mask & (1u << u)) __builtin_amdgcn_raw_buffer_store_b64(w, rb.rs, vo, so, 0);
      else __builtin_amdgcn_raw_buffer_store_b64(w, rb.rs, vo, so, BUF_NT);
    } else {
      if (mask & (1u << u)) __builtin_amdgcn_raw_buffer_store_b32(w, rb.rs, vo, so, 0);
      else __builtin_amdgcn_raw_buffer_store_b32(w, rb.rs, vo, so, BUF_NT);
    }
  }
}
#else
// host pass of hipcc: the kernels' bodies are parsed but never emitted -- declarations only
template <int IO> struct RowBufT { unsigned vo, su, rowb; };
using RowBuf = RowBufT<0>;
template <int IO> __device__ cf widen2(unsigned w);
template <int IO> __device__ unsigned narrow2(float fx, float fy);
template <int IO = 0>
__device__ RowBufT<IO> row_buf(const void* row0, const Geom& g, int t, int d, bool in_range = true);
template <int IO>
__device__ RowBufT<IO> row_buf(const void* base, int b, const Geom& g, int t, int d, bool in_range = true);
template <int U0, int CNT, bool PAD, int IO> __device__ void load_rows(const RowBufT<IO>& rb, int r, cf (&v)[16]);
__device__ unsigned st_tile_mask(const DecimArgs& a, int r, int sw);
template <bool PAD, int IO> __device__ void store_rows(const RowBufT<IO>& rb, int r, const cf (&v)[16], unsigned mask);
#endif

// ---- launch helpers ----------------------------------------------------------------------------
static inline int n_wg(const DecimArgs& a) { return a.g.B * ((a.g.D + DT - 1) / DT); }

// Run-time values -> template arguments (the spelling of row_dispatch, smx_rows.h).  pick<Vs...>(v, f) calls
// f(std::integral_constant<int, V>()) for the V == v and hands back what f returns; no such V: false.
template <int... Vs, class F>
bool pick(int v, F&& f) {
  return ((v == Vs && f(std::integral_constant<int, Vs>())) || ...);
}
template <class F>
bool pick_bool(bool v, F&& f) {
  return v ? f(std::true_type()) : f(std::false_type());
}
// A whole template key at once: pick_key(f, among<1, 2, 4>{nb}, among<0, 1, 2>{mode}, flag{pad}) calls f(NB, MODE, PAD)
// with the constants in that order and returns true; a value outside its list: f is not called, false.  f launches under
// `if constexpr (<family>_instance(...))`, the constexpr predicate next to the kernel that states which instances exist
// -- so of the cross product only those are emitted -- and returns true either way: the launcher has asked the same
// predicate at run time before its first launch (a key without an instance is hipErrorInvalidValue, never a
// neighbouring instance), so the empty branch is never reached.
// SMX_KEY(NB) = the constant's value (a parameter of the generic lambda is not a constant expression itself).
// (among<Vs...>, flag: smx_kernels.h)
#define SMX_KEY(v) decltype(v)::value
template <class F>
bool pick_key(F&& f) { return f(); }
template <class F, int... Vs, class... Ks>
bool pick_key(F&& f, among<Vs...> k, Ks... rest);
template <class F, class... Ks>
bool pick_key(F&& f, flag k, Ks... rest) {
  return pick_bool(k.v, [&](auto V) { return pick_key([&](auto... vs) { return f(V, vs...); }, rest...); });
}
template <class F, int... Vs, class... Ks>
bool pick_key(F&& f, among<Vs...> k, Ks... rest) {
  return pick<Vs...>(k.v, [&](auto V) { return pick_key([&](auto... vs) { return f(V, vs...); }, rest...); });
}

// The one launch statement of the transform families: SMX_LAUNCH((k_fused<NB, MODE>), grid, block, stream, args...).
// With SMX_LAUNCH_TRACE defined (tests/launch_trace only, never in build.sh) nothing reaches the HIP runtime: the
// instance's name, the grid and block, and bid0 of a DecimArgs argument go to trace_launch, which the test program defines.
#ifdef SMX_LAUNCH_TRACE
template <auto K> struct KTag {};          // typeid(KTag<K>).name() carries every template argument of K
void trace_launch(const char* ktag, dim3 grid, dim3 block, const DecimArgs* a);
template <class A0, class... A>
const DecimArgs* trace_decim(const A0& a0, const A&...) {
  if constexpr (std::is_same_v<A0, DecimArgs>) return &a0; else return nullptr;
}
#define SMX_LAUNCH(K, grid, block, s, ...) \
  ::smx::trace_launch(typeid(::smx::KTag<(K)>).name(), grid, block, ::smx::trace_decim(__VA_ARGS__))
static inline hipError_t launch_status() { return hipSuccess; }
#else
#define SMX_LAUNCH(K, grid, block, s, ...) hipLaunchKernelGGL(K, grid, block, 0, s, __VA_ARGS__)
static inline hipError_t launch_status() { return hipGetLastError(); }
#endif

// The streaming kernels are launched in rounds of `a.round` workgroups (512 = 2 per CU, all resident):
// the kernel boundary keeps every round's read phase and write phase chip-wide in step.  One launch of
// 1024 workgroups lets the second round's reads run into the first round's writes, and mixed traffic is
// slower on this HBM.  Measured gain is small (1-2 % at (64,4096,512), (128,4096,256) and C3); the
// four-band kernels (one workgroup per CU) are faster in a single launch and keep that.
template <typename F>
static inline hipError_t for_rounds(const DecimArgs& a, int total, F launch, bool single = false) {
  const int round = a.round > 0 && !single ? a.round : total;
  for (int b0 = 0; b0 < total; b0 += round) {
    DecimArgs r = a;
    r.bid0 = b0;
    launch(r, dim3(total - b0 < round ? total - b0 : round));
  }
  return launch_status();
}

}  // namespace smx
