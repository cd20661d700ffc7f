// smx_decim.hip -- decimated, output-pruned Stockham kernels for gfx950 (N = 256 L, k <= 512).
//
// Workgroup = 256 threads = 16 row-groups t x 16 packed channel pairs j, owning (batch row b,
// 32 channels).  A global row is 128 contiguous bytes per workgroup (16 lanes x float2), so every
// wave instruction moves 4 full 128-B segments.  x is read once, y is written once; the only
// other HBM traffic is the (B,k,D) spectrum (N/k times smaller than x).
//
// Replaces: reference fft_tensor/spectral_layers.py:88 (fft), :94-109 (filter), :112-116 (ifft, bias)
// and the autograd backward of the same lines.
#include "smx_launch.h"

namespace smx {

template <int NB>
__device__ __forceinline__ void zero_acc(TState<NB>& st) {
#pragma unroll
  for (int s = 0; s < 16 * NB; ++s) st.acc[s] = mk(0.f, 0.f);
}

// unpack + filter between the two loops, in LDS rounds of 32 slots (UnpackRounds in smx_core.h).
// Enters and leaves with the LDS free (barriers included).
template <int NB, int MODE, bool BATCHED, int ROUND>
__device__ __forceinline__ void unpack_round(TState<NB>& st, cf* lds, const Geom& g,
                                             const FilterArgs& fa, int b, int d, bool valid, int t,
                                             int j, const ZSave<NB>& zs, const WPre* wp, cf* gs) {
  if constexpr (ROUND < UnpackRounds<NB>::N) {
    __syncthreads();
    unpack_phase1<NB, ROUND>(st, lds, t, j);
    const cf* wl = nullptr;
    if constexpr (NB == 1 && MODE != 2) {
      if (wp) { stage_w(*wp, lds + EX, t * 16 + j, fa.conj_w); wl = lds + EX; }
    }
    __syncthreads();
    if constexpr (BATCHED) unpack_phase2_batched<NB, MODE, ROUND>(st, lds, g, fa, b, d, valid, t, j, zs, gs, wl);
    else unpack_phase2<NB, MODE, ROUND>(st, lds, g, fa, b, d, valid, t, j, zs, wl, gs);
    unpack_round<NB, MODE, BATCHED, ROUND + 1>(st, lds, g, fa, b, d, valid, t, j, zs, wp, gs);
  }
}

template <int NB, int MODE, bool BATCHED>
__device__ __forceinline__ void unpack_filter(TState<NB>& st, cf* lds, const Geom& g,
                                              const FilterArgs& fa, int b, int d, bool valid, int t,
                                              int j, const WPre* wp = nullptr) {
  const ZSave<NB> zs = save_z<NB>(st);
  // two bands, backward: the 16 rows of the saved spectrum this thread needs are requested here in one
  // burst (the tile registers of the loops are dead by now) and the slab rows leave right after the
  // unpack -- not as dependent load -> store pairs inside the slot loop
  if constexpr (NB == 2 && MODE == 1 && !BATCHED) prefetch_io<NB, MODE>(st, g, fa, b, d, valid, t);
  cf gs = mk(0.f, 0.f);                 // gradient of the per-row filter factor (summed unconditionally: a
  const bool want_gs = MODE == 1 && fa.gsc != nullptr;         // run-time pointer would push it to scratch)
  unpack_round<NB, MODE, BATCHED, 0>(st, lds, g, fa, b, d, valid, t, j, zs, wp, MODE == 1 ? &gs : nullptr);
  if constexpr (NB == 2 && MODE == 1 && !BATCHED) store_io<NB, MODE>(st, g, fa, b, d, valid, t);
  if constexpr (MODE == 1) {
    if (want_gs) {               // the 16 threads that share a channel pair: fixed-order sum through LDS
      __syncthreads();
      lds[t * 16 + j] = gs;
      __syncthreads();
      if (t == 0 && valid) {
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) { sa += lds[u * 16 + j].x; sb += lds[u * 16 + j].y; }
        fa.gsc[(size_t)b * g.D + d] = sa;
        fa.gsc[(size_t)b * g.D + d + 1] = sb;
      }
    }
  }
}

// LayerNorm folded into the load (fused block only): per-row (mean, rstd) and this thread's two
// channels of gamma / beta.  st[u] belongs to row (16 u + t) L + r, like the tile itself.
struct LnLoad {
  const cf* sb;          // stats of batch row b, (N)
  float g0, g1, b0, b1;
};
template <int U0, int CNT>
__device__ __forceinline__ void load_stats(const cf* __restrict__ sb, const Geom& g, int t, int r,
                                           cf (&sv)[16]) {
  const cf* p = sb + (size_t)t * g.L + r;
#pragma unroll
  for (int u = U0; u < U0 + CNT; ++u) sv[u] = p[(size_t)u * 16 * g.L];
}

// One tile of the forward half.  LAST = no tile follows (nothing is prefetched): the loops below peel their last
// iteration instead of guarding the prefetches with `if (i + 1 < cnt)` -- with the guards the register allocator
// put the copies of the conditionally loaded registers right behind the loads (s_waitcnt vmcnt(7) eight
// instructions after the burst: the whole memory latency exposed once per tile).
// DROP (backward launches): the tile is g, multiplied by the dropout mask of the forward pass as it
// is moved into the working registers.  pj = this thread's pair index inside a row, (d >> 1).
template <int NB, bool LN, bool DROP, bool PAD, bool LAST, class XB>
__device__ __forceinline__ void forward_tile(TState<NB>& st, cf* E, const XB& xb,
                                             const DecimArgs& a, int t, int j, int r, int rn, cf (&nx)[16],
                                             cf (&ns)[LN ? 16 : 1], const LnLoad* ln, Drop dr, unsigned pj) {
  const Geom& g = a.g;
  if constexpr (LN) {
#pragma unroll
    for (int u = 0; u < 16; ++u)
      st.v[u] = mk(fmaf((nx[u].x - ns[u].x) * ns[u].y, ln->g0, ln->b0),
                   fmaf((nx[u].y - ns[u].x) * ns[u].y, ln->g1, ln->b1));
  } else if constexpr (DROP) {
    const unsigned hd = (unsigned)(g.D >> 1), pstride = 16u * (unsigned)g.L * hd;
    const unsigned p0 = ((unsigned)t * (unsigned)g.L + (unsigned)r) * hd + pj;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      st.v[u] = drop_apply(nx[u], drop_hash(p0 + (unsigned)u * pstride, dr.key), dr.thr, dr.scale);
  } else {
#pragma unroll
    for (int u = 0; u < 16; ++u) st.v[u] = nx[u];
  }
  // The next tile's 16 loads go out in two bursts, before and after the exchange barrier:
  // smoother request issue measured ~3 us faster per launch than one 16-load burst (and than four).
  if constexpr (!LAST) {
    load_rows<0, 8, PAD>(xb, rn, nx);
    if constexpr (LN) load_stats<0, 8>(ln->sb, g, t, rn, ns);
    __builtin_amdgcn_sched_barrier(0);       // (the scheduler otherwise sinks this burst below the transform)
  }
  fwd_phase1_cp<NB>(st, E, t, j);
  // the next tile's inter-pass twiddles, into the registers this tile's products have just freed
  if constexpr (!LAST) load_cp(a.tq + ((size_t)t * g.L + rn) * 16, st.cp);
  __syncthreads();
  if constexpr (!LAST) {
    load_rows<8, 8, PAD>(xb, rn, nx);
    if constexpr (LN) load_stats<8, 8>(ln->sb, g, t, rn, ns);
  }
  fwd_phase2<NB, true>(st, E, a.bt + (size_t)r * BT_STRIDE, t, j);
}

// forward half: accumulate residues [rbeg, rbeg+cnt) (visited in rotated order) into st.acc.
template <int NB, bool LN = false, bool DROP = false, bool PAD = false, class XB>
__device__ __forceinline__ void forward_loop(TState<NB>& st, cf* lds, const XB& xb,
                                             const DecimArgs& a, int t, int j, int rbeg, int cnt,
                                             int rot, const LnLoad* ln = nullptr, Drop dr = Drop{},
                                             unsigned pj = 0) {
  const Geom& g = a.g;
  const int rend = rbeg + cnt;
  // One tile is prefetched in registers while the previous one is transformed.  (Two tiles ahead
  // was measured slower twice: the memory system is already saturated, deeper queues only add latency.)
  cf nx[16];
  cf ns[LN ? 16 : 1];
  int r = rbeg + rot;
  load_rows<0, 16, PAD>(xb, r, nx);
  if constexpr (LN) load_stats<0, 16>(ln->sb, g, t, r, ns);
  // inter-pass twiddles c^q = w_N^{q (L t + r)} from row (t, r) of the table tq (round 4; rounds 1-3 raised
  // c to its powers per tile: 56 of the loop's 530 vector instructions), one tile ahead like the tile itself
  load_cp(a.tq + ((size_t)t * g.L + r) * 16, st.cp);
  int i = 0;
  for (; i + 1 < cnt; ++i) {
    int rn = r + 1;
    if (rn == rend) rn = rbeg;
    forward_tile<NB, LN, DROP, PAD, false>(st, lds + (i & 1) * EX, xb, a, t, j, r, rn, nx, ns, ln, dr, pj);
    r = rn;
  }
  forward_tile<NB, LN, DROP, PAD, true>(st, lds + (i & 1) * EX, xb, a, t, j, r, r, nx, ns, ln, dr, pj);
}

// One tile of the inverse half.  No vector-memory LOAD may sit between a tile's stores and the next use of loaded
// data: vmcnt counts loads and stores in one in-order queue, so waiting for such a load means waiting for every
// store issued before it (rounds 1-3 read the per-residue twiddles with per-lane loads at the top of each
// iteration and so drained the previous tile's 16 stores before computing anything).  The per-residue twiddles now
// come through the scalar cache, and the next tile's c^q row is requested BEFORE this tile's stores (st.cp is dead
// once the gather has multiplied by it).
// RES: add the rows of `res` (the block input x, same addressing as the output) before the store;
// the rows of the next tile are fetched while the current one is transformed.  (Walking the residues
// in reverse with cacheable loads, so that the second read of x would hit the 256 MiB Infinity
// Cache, was measured: no gain inside a fwd+bwd sequence -- tools/probe_mall.hip shows re-reads at
// HBM rate whatever the footprint.)
// DROP (forward launches): dropout of the tile before the residual add and the store.
template <int NB, bool RES, bool DROP, bool PAD, bool LAST, class YB, class RB>
__device__ __forceinline__ void inverse_tile(TState<NB>& st, cf* E, const YB& yb, const DecimArgs& a,
                                             int t, int j, int r, int rn,
                                             const RB& res, cf (&rx)[RES ? 16 : 1], Drop dr,
                                             unsigned pj, int sw) {
  const Geom& g = a.g;
  inv_phase1<NB, true>(st, a.bt + (size_t)r * BT_STRIDE, E, t, j);
  __syncthreads();
  inv_phase2_gather<NB>(st, E, t, j);
  if constexpr (!LAST) {
    // pinned between the last use of st.cp and the stores: hoisted above the gather the loads need registers of
    // their own and copies at the loop's end -- behind the stores, i.e. a wait for them
    __builtin_amdgcn_sched_barrier(0);
    load_cp(a.tq + ((size_t)t * g.L + rn) * 16, st.cp);
    __builtin_amdgcn_sched_barrier(0);
  }
  fft16<+1>(st.v);
  if constexpr (DROP) {
    const unsigned hd = (unsigned)(g.D >> 1), pstride = 16u * (unsigned)g.L * hd;
    const unsigned p0 = ((unsigned)t * (unsigned)g.L + (unsigned)r) * hd + pj;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      st.v[u] = drop_apply(st.v[u], drop_hash(p0 + (unsigned)u * pstride, dr.key), dr.thr, dr.scale);
  }
  if constexpr (RES) {
#pragma unroll
    for (int u = 0; u < 16; ++u) st.v[u] = cadd(st.v[u], rx[u]);
    if constexpr (!LAST) load_rows<0, 16, PAD>(res, rn, rx);
  }
  store_rows<PAD>(yb, r, st.v, st_tile_mask(a, r, sw));
}

template <int NB, bool RES = false, bool DROP = false, bool PAD = false, class YB, class RB>
__device__ __forceinline__ void inverse_loop(TState<NB>& st, cf* lds, const YB& yb,
                                             const DecimArgs& a, int t, int j, int rbeg,
                                             int cnt, int rot, const RB& res, Drop dr = Drop{},
                                             unsigned pj = 0) {
  const Geom& g = a.g;
  int r = rbeg + rot;
  // the wave's term of the store layout's rotation (st_tile_mask, smx_launch.h): scalar, formed once
  const int sw = (__builtin_amdgcn_readfirstlane(t) >> 2) >> a.st_wsh;      // (the wave's first lane has t = 4 w)
  cf rx[RES ? 16 : 1];
  if constexpr (RES) load_rows<0, 16, PAD>(res, r, rx);
  load_cp(a.tq + ((size_t)t * g.L + r) * 16, st.cp);
  // The first row is waited for HERE, so that the loop is entered with nothing in flight: the compiler's wait counts
  // inside the loop are the stricter of "entered from above" and "came round the back edge", and with these eight
  // loads pending on entry every iteration would wait vmcnt(0) for its twiddles -- i.e. for the previous tile's stores
  // -- instead of vmcnt(16).  (An L2 hit, once per launch.)
  __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0), gfx9 encoding
  int i = 0;
  for (; i + 1 < cnt; ++i) {
    int rn = r + 1;
    if (rn == rbeg + cnt) rn = rbeg;
    inverse_tile<NB, RES, DROP, PAD, false>(st, lds + (i & 1) * EX, yb, a, t, j, r, rn, res, rx, dr, pj, sw);
    r = rn;
  }
  inverse_tile<NB, RES, DROP, PAD, true>(st, lds + (i & 1) * EX, yb, a, t, j, r, r, res, rx, dr, pj, sw);
}

__device__ __forceinline__ Drop make_drop(const DecimArgs& a, int b) {
  Drop dr;
  dr.thr = a.drop_thr; dr.scale = a.drop_scale;
  dr.key = drop_row_key(a.rng[0], a.rng[1], b);
  return dr;
}

// ---- fused: one launch per direction ----------------------------------------------------------
// ACC (band groups after the first, k > 512): the launch adds its bins' contribution to what the
// earlier groups stored, read-modify-write per tile by the workgroup that owns it.
// PAD: x / y hold R < N rows (zero-padded transform, cropped output).
// IO: element type of the streamed rows of a.in / a.out (RowBufT, smx_launch.h): 0 f32, 1 bf16, 2 fp16.  Only the row
// I/O differs: the same work items and residue rotation (wg_map -- the order in which a workgroup accumulates its
// residues), the same tile arithmetic, f32 spectra.  The 2-byte results are therefore the f32 kernel's results on
// the widened input, rounded once at the store.  Only the configurations smx_api routes there
// are instantiated (launch_fused).  Parameter gradients are never reduced here: every backward leaves its slab rows
// and bias partials for a launch of its own (k_gradw_slab).
// OIO: element type of a.out where it is not a.in's.  One pairing exists: 2-byte g in, f32 rows out (MODE 1), the
// transform of the 2-byte block backward -- its output is grad_h, which the LayerNorm backward reads unrounded.
// The instances of k_fused that exist (launch_fused asks this before it launches, and instantiates nothing else).
// 2-byte rows (io = SMX_IO_BF16 / SMX_IO_F16): only what smx_api routes to them -- modes 0 and 1 with and without dropout,
// no zero-padded rows, no accumulating band groups; f32 rows out of 2-byte g (oio 0) in mode 1 only, the block backward.
// An f32 instance must never read 2-byte rows.
constexpr bool fused_instance(int nb, int mode, bool drop, bool acc, bool pad, int io, int oio) {
  if (!among<1, 2, 4>::has(nb) || !among<0, 1, 2>::has(mode)) return false;
  if (acc) return nb == 4 && mode != 2 && !drop && io == 0 && oio == 0;   // band groups after the first: four bands
  if (io == 0) return oio == 0 && !(drop && (pad || mode == 2));          // (dropout never with zero-padded rows)
  return among<1, 2>::has(io) && mode != 2 && !pad && (oio == io || (oio == 0 && mode == 1));
}
template <int NB, int MODE, bool DROP = false, bool ACC = false, bool PAD = false, int IO = 0, int OIO = IO>
__global__ __launch_bounds__(TPB, 2) void k_fused(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, 1, g.L, a.placement);
  const int b = w.b, d = w.dt * DT + 2 * j, rot = w.rot;
  const bool valid = d < g.D;
  RowBufT<IO> xb;
  if constexpr (IO == 0) xb = row_buf(a.in + (size_t)b * g.R * g.D, g, t, valid ? d : g.D - 2);
  else xb = row_buf<IO>(a.in, b, g, t, valid ? d : g.D - 2);

  TState<NB> st;
  zero_acc<NB>(st);
  if constexpr (NB == 1) prefetch_io<NB, MODE>(st, g, a.fa, b, d, valid, t);   // saved spectrum, see smx_core.h
  WPre wp;
  constexpr bool STAGE_W = NB == 1 && MODE != 2;           // filter slice via LDS, see prefetch_w
  if constexpr (STAGE_W) prefetch_w(wp, g, a.fa.w_re, a.fa.w_im, w.dt * DT, tid);
  Drop dr{};
  if constexpr (DROP) dr = make_drop(a, b);
  const unsigned pj = (unsigned)((valid ? d : g.D - 2) >> 1);
  // SMX_AB_*: timing ablations for tools/ab.sh (wrong results by design; never defined in the shipped build)
#ifndef SMX_AB_NO_FWD
  forward_loop<NB, false, DROP && MODE == 1, PAD>(st, lds, xb, a, t, j, 0, g.L, rot, nullptr, dr, pj);
#endif
#ifndef SMX_AB_NO_UNPACK
  unpack_filter<NB, MODE, false>(st, lds, g, a.fa, b, d, valid, t, j, STAGE_W ? &wp : nullptr);
#endif
#ifdef SMX_AB_NO_INV
  if (st.acc[0].x == 12345.f) a.out[0] = st.acc[1].y;     // keeps the first half alive
  return;
#endif
  if (a.out == nullptr) {
    if constexpr (NB == 1) store_io<NB, MODE>(st, g, a.fa, b, d, valid, t);
    // phase-split backward: park the filtered spectrum for k_split_b (same layout as k_split_f)
    if (a.ws_s != nullptr) {
      cf* s = a.ws_s + (size_t)(b * ndt + w.dt) * (16 * NB * TPB);
#pragma unroll
      for (int sl = 0; sl < 16 * NB; ++sl) s[sl * TPB + tid] = st.acc[sl];
    }
    return;
  }
  __syncthreads();
  RowBufT<OIO> yb;   // (ACC: also read back)
  if constexpr (OIO == 0) yb = row_buf(a.out + (size_t)b * g.R * g.D, g, t, d, valid);
  else yb = row_buf<OIO>(a.out, b, g, t, d, valid);
  inverse_loop<NB, ACC, DROP && MODE == 0, PAD>(st, lds, yb, a, t, j, 0, g.L, rot, yb, dr, pj);
  if constexpr (NB == 1) store_io<NB, MODE>(st, g, a.fa, b, d, valid, t);     // saved spectrum / grad slab
}

// ---- sixteen-row decimation: N = 16 P, any P (smx_core.h) ------------------------------------------------
// The loops walk tiles of 16 residues [tbeg, tbeg + cnt), starting at tbeg + rot.  DROP: the fused dropout of the
// 256-point kernels -- the mask of element pair (row n, channel pair) is a hash of (n D/2 + d/2, key of the batch
// row); forward launches apply it to the stored tile, backward launches to the loaded g.
template <int NB, bool PAD, bool DROP>
__device__ __forceinline__ void forward16_loop(TState<NB>& st, cf* lds, const float* __restrict__ xb,
                                               const DecimArgs& a, int t, int j, int tbeg, int cnt, int rot,
                                               Drop dr, unsigned pj) {
  const Geom& g = a.g;
  const unsigned hd = (unsigned)(g.D >> 1);
  cf nx[16];
  int tau = tbeg + rot;
  load_tile16<PAD>(xb, g, t, tau, nx);
  cf cn = a.tw[min(16 * tau + t, g.N - 1)];
  for (int i = 0; i < cnt; ++i) {
    if constexpr (DROP) {
      const unsigned p0 = (unsigned)(16 * tau + t) * hd + pj, ps = (unsigned)g.P * hd;
#pragma unroll
      for (int u = 0; u < 16; ++u)
        st.v[u] = drop_apply(nx[u], drop_hash(p0 + (unsigned)u * ps, dr.key), dr.thr, dr.scale);
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) st.v[u] = nx[u];
    }
    const cf c = cn;
    int tn = tau + 1;
    if (tn == tbeg + cnt) tn = tbeg;
    if (i + 1 < cnt) {
      load_tile16<PAD>(xb, g, t, tn, nx);
      cn = a.tw[min(16 * tn + t, g.N - 1)];
    }
    cf* E = lds + (i & 1) * EX;
    fwd_phase1<NB>(st, c, E, t, j);                       // fft16 over the 16 rows, times w_N^{q r}, scatter
    __syncthreads();
    fwd16_phase2<NB>(st, E, a.v16, a.b16 + (size_t)tau * 32, t, j);
    tau = tn;
  }
}
template <int NB, bool PAD, bool DROP>
__device__ __forceinline__ void inverse16_loop(TState<NB>& st, cf* lds, float* __restrict__ yb, const DecimArgs& a,
                                               int t, int j, bool valid, int tbeg, int cnt, int rot, Drop dr,
                                               unsigned pj) {
  const Geom& g = a.g;
  const unsigned hd = (unsigned)(g.D >> 1);
  int tau = tbeg + rot;
  for (int i = 0; i < cnt; ++i) {
    const cf c = a.tw[min(16 * tau + t, g.N - 1)];
    cf* E = lds + (i & 1) * EX;
    inv16_phase1<NB>(st, a.v16, a.b16 + (size_t)tau * 32, E, t, j);
    __syncthreads();
    inv_phase2<NB>(st, c, E, t, j);                       // gather, times w_N^{-q r}, inverse fft16 -> the 16 rows
    if constexpr (DROP) {
      const unsigned p0 = (unsigned)(16 * tau + t) * hd + pj, ps = (unsigned)g.P * hd;
#pragma unroll
      for (int u = 0; u < 16; ++u)
        st.v[u] = drop_apply(st.v[u], drop_hash(p0 + (unsigned)u * ps, dr.key), dr.thr, dr.scale);
    }
    store_tile16<PAD>(yb, g, t, tau, valid, st.v);
    ++tau;
    if (tau == tbeg + cnt) tau = tbeg;
  }
}

// One launch per direction like k_fused<NB, MODE>.  NB = 1: k <= 128, the filter slice staged through LDS;
// NB = 2: k <= 256, the filter from its packed copy (fa.wt) or gathered.
constexpr bool fused16_instance(int nb, int mode, bool pad, bool drop) {
  return among<1, 2>::has(nb) && among<0, 1, 2>::has(mode) && !(drop && (pad || mode == 2));
}
template <int NB, int MODE, bool PAD = false, bool DROP = false>
__global__ __launch_bounds__(TPB, 2) void k_fused16(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const int T = g.L;                                      // tiles
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, 1, T, a.placement);
  const int b = w.b, d = w.dt * DT + 2 * j, rot = w.rot;
  const bool valid = d < g.D;
  const float* xb = a.in + (size_t)b * g.R * g.D + (valid ? d : g.D - 2);
  TState<NB> st;
  zero_acc<NB>(st);
  if constexpr (NB == 1) prefetch_io<NB, MODE>(st, g, a.fa, b, d, valid, t);
  WPre wp;
  constexpr bool STAGE_W = NB == 1 && MODE != 2;
  if constexpr (STAGE_W) prefetch_w(wp, g, a.fa.w_re, a.fa.w_im, w.dt * DT, tid);
  Drop dr{};
  if constexpr (DROP) dr = make_drop(a, b);
  const unsigned pj = (unsigned)((valid ? d : g.D - 2) >> 1);
  forward16_loop<NB, PAD, DROP && MODE == 1>(st, lds, xb, a, t, j, 0, T, rot, dr, pj);
  unpack_filter<NB, MODE, false>(st, lds, g, a.fa, b, d, valid, t, j, STAGE_W ? &wp : nullptr);
  if (a.out == nullptr) {
    if constexpr (NB == 1) store_io<NB, MODE>(st, g, a.fa, b, d, valid, t);
    if (a.ws_s != nullptr) {          // phase-split backward: park the filtered spectrum for k_split16_b
      cf* sp = a.ws_s + (size_t)(b * ndt + w.dt) * (16 * NB * TPB);
#pragma unroll
      for (int sl = 0; sl < 16 * NB; ++sl) sp[sl * TPB + tid] = st.acc[sl];
    }
    return;
  }
  __syncthreads();
  inverse16_loop<NB, PAD, DROP && MODE == 0>(st, lds, a.out + (size_t)b * g.R * g.D + d, a, t, j, valid, 0, T, rot, dr,
                                             pj);
  if constexpr (NB == 1) store_io<NB, MODE>(st, g, a.fa, b, d, valid, t);
}

// Few (batch row, d-tile) pairs: the tiles are cut into nsplit chunks as on the 256-point split plan -- (A) partial
// spectra per chunk, then the SAME k_split_sum / k_split_f (the accumulator layout is the same), then (B) the inverse
// per chunk.  (B) with nsplit = 1 is also the inverse half of a phase-split backward.
constexpr bool split16_instance(int nb, bool pad, bool drop) {      // k_split16_a and k_split16_b
  return among<1, 2>::has(nb) && !(pad && drop);
}
template <int NB, bool PAD = false, bool DROP = false>
__global__ __launch_bounds__(TPB, 2) void k_split16_a(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, a.nsplit, a.lc, a.placement);
  const int c = w.c, b = w.b, wg = b * ndt + w.dt, d = w.dt * DT + 2 * j;
  const bool valid = d < g.D;
  const int tbeg = c * a.lc, cnt = min(a.lc, g.L - tbeg);
  const float* xb = a.in + (size_t)b * g.R * g.D + (valid ? d : g.D - 2);
  TState<NB> st;
  zero_acc<NB>(st);
  Drop dr{};
  if constexpr (DROP) dr = make_drop(a, b);
  if (cnt > 0)
    forward16_loop<NB, PAD, DROP>(st, lds, xb, a, t, j, tbeg, cnt, w.rot % cnt, dr,
                                  (unsigned)((valid ? d : g.D - 2) >> 1));
  cf* z = a.ws_z + ((size_t)wg * a.nsplit + c) * (16 * NB * TPB);
#pragma unroll
  for (int sl = 0; sl < 16 * NB; ++sl) z[sl * TPB + tid] = st.acc[sl];
}
template <int NB, bool PAD = false, bool DROP = false>
__global__ __launch_bounds__(TPB, 2) void k_split16_b(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, a.nsplit, a.lc, a.placement);
  const int c = w.c, b = w.b, wg = b * ndt + w.dt, d = w.dt * DT + 2 * j;
  const bool valid = d < g.D;
  const int tbeg = c * a.lc, cnt = min(a.lc, g.L - tbeg);
  if (cnt <= 0) return;
  TState<NB> st;
  const cf* sp = a.ws_s + (size_t)wg * (16 * NB * TPB);
#pragma unroll
  for (int sl = 0; sl < 16 * NB; ++sl) st.acc[sl] = sp[sl * TPB + tid];
  Drop dr{};
  if constexpr (DROP) dr = make_drop(a, b);
  inverse16_loop<NB, PAD, DROP>(st, lds, a.out + (size_t)b * g.R * g.D + d, a, t, j, valid, tbeg, cnt, w.rot % cnt, dr,
                                (unsigned)((valid ? d : g.D - 2) >> 1));
}

// ---- synthesis from a given one-sided spectrum (smx_irfft_ex): the inverse half alone ---------------
// The accumulators are filled from the rows of the (B,k,D) spectrum (synth_fill: no exchange, no filter) and
// the inverse loop runs as in k_fused; with out == NULL they are parked for k_split_b (residue-split plans).
template <int NB, bool PAD>
__global__ __launch_bounds__(TPB, 2) void k_synth(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, 1, g.L, a.placement);
  const int b = w.b, d = w.dt * DT + 2 * j, rot = w.rot;
  const bool valid = d < g.D;
  TState<NB> st;
  synth_fill<NB>(st, g, a.fa, b, d, valid, t);
  if (a.out == nullptr) {
    cf* s = a.ws_s + (size_t)(b * ndt + w.dt) * (16 * NB * TPB);
#pragma unroll
    for (int sl = 0; sl < 16 * NB; ++sl) s[sl * TPB + tid] = st.acc[sl];
    return;
  }
  const RowBuf yb = row_buf(a.out + (size_t)b * g.R * g.D, g, t, d, valid);
  inverse_loop<NB, false, false, PAD>(st, lds, yb, a, t, j, 0, g.L, rot, yb);
}

// ---- full spectrum at N = 2048: eight bands, one launch per direction ------------------------------
// The whole packed spectrum of the workgroup's 16 channel pairs lives in registers (128 complex per
// thread, partly in AGPRs: one workgroup per CU).  Eight tiles with compile-time residues: each tile's
// 256-point spectrum is kept apart (fwd_phase2_store), an 8-point transform across the residues turns
// them into the eight bands, the unpack runs in four LDS rounds, and the inverse mirrors it.  Replaces
// two band-group launches per direction + three edge-bin passes (each group re-reading x and
// re-writing y) for the reference's default causal-convolution lengths (seq_len 1024 + kernel 128 ->
// n_fft 2048, fft_lm/train_fixed_full.py:507-519).
template <int R, int MODE, bool PAD>
__device__ __forceinline__ void full8_fwd_tiles(TState<8>& st, cf* lds, const float* __restrict__ xb,
                                                const DecimArgs& a, int t, int j, cf (&nx)[16], cf& cn) {
  if constexpr (R < 8) {
    const Geom& g = a.g;
#pragma unroll
    for (int u = 0; u < 16; ++u) st.v[u] = nx[u];
    const cf c = cn;
    if constexpr (R + 1 < 8) {
      load_part_tile<0, 8, PAD>(xb, g, t, R + 1, nx);
      cn = a.tw[(size_t)t * 8 + R + 1];
    }
    cf* E = lds + (R & 1) * EX;
    fwd_phase1<8>(st, c, E, t, j);
    __syncthreads();
    if constexpr (R + 1 < 8) load_part_tile<8, 8, PAD>(xb, g, t, R + 1, nx);
    fwd_phase2_store<8, R>(st, E, a.bt + (size_t)R * BT_STRIDE, t, j);
    full8_fwd_tiles<R + 1, MODE, PAD>(st, lds, xb, a, t, j, nx, cn);
  }
}
template <int R, bool PAD>
__device__ __forceinline__ void full8_inv_tiles(TState<8>& st, cf* lds, float* __restrict__ yb,
                                                const DecimArgs& a, int t, int j, bool valid) {
  if constexpr (R < 8) {
    const cf c = a.tw[(size_t)t * 8 + R];
    cf* E = lds + (R & 1) * EX;
    inv_phase1_from<8, R>(st, a.bt + (size_t)R * BT_STRIDE, E, t, j);
    __syncthreads();
    inv_phase2<8>(st, c, E, t, j);
    store_tile<PAD>(yb, a.g, t, R, valid, st.v);
    full8_inv_tiles<R + 1, PAD>(st, lds, yb, a, t, j, valid);
  }
}

template <int MODE, bool PAD>
__global__ __launch_bounds__(TPB, 1) void k_full8(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, 1, g.L, a.placement);
  const int b = w.b, d = w.dt * DT + 2 * j;
  const bool valid = d < g.D;
  const float* xb = a.in + (size_t)b * g.R * g.D + (valid ? d : g.D - 2);

  TState<8> st;
  cf nx[16];
  load_tile<PAD>(xb, g, t, 0, nx);
  cf cn = a.tw[(size_t)t * 8];
  full8_fwd_tiles<0, MODE, PAD>(st, lds, xb, a, t, j, nx, cn);
  residue_fft8<-1>(st);
#ifndef SMX_FULL8_BATCHED
#define SMX_FULL8_BATCHED false
#endif
  // (the batched unpack of k_split_f spills ~1700 registers here; the slot loop prefetches instead)
  unpack_filter<8, MODE, SMX_FULL8_BATCHED>(st, lds, g, a.fa, b, d, valid, t, j);
  if (a.out == nullptr) return;                      // spectrum only / parameter gradients only
  __syncthreads();
  residue_fft8<+1>(st);
  full8_inv_tiles<0, PAD>(st, lds, a.out + (size_t)b * g.R * g.D + d, a, t, j, valid);
}

// synthesis at N = 2048 from a given one-sided spectrum: the eight bands filled from its rows (synth_fill<8>),
// bands -> residues, inverse tiles -- one launch, the spectrum read once and y written once
template <bool PAD>
__global__ __launch_bounds__(TPB, 1) void k_synth8(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, 1, g.L, a.placement);
  const int b = w.b, d = w.dt * DT + 2 * j;
  const bool valid = d < g.D;
  TState<8> st;
  synth_fill<8>(st, g, a.fa, b, d, valid, t);
  residue_fft8<+1>(st);
  full8_inv_tiles<0, PAD>(st, lds, a.out + (size_t)b * g.R * g.D + d, a, t, j, valid);
}

// ---- fused block: y = x + mix(LayerNorm(x)) in one launch (reference spectral_layers.py:185) ------
// Same structure as k_fused<NB, 0>; x is read a second time at the store for the residual.
// (four bands: 256 VGPRs are not enough for the extra row statistics and residual rows -- 57 spills
// inside the loops cost more than the second workgroup per CU gains: 784 vs 688 us at (32,4096,1024))
// IO: element type of x and y as in k_fused -- the LayerNorm-on-load rows, the residual re-read and the store; the
// statistics, gamma / beta and the spectrum stay f32, so y is the f32 kernel's y on the widened x, rounded once.
// k_fused_blk<NB, DROP, IO>: every combination of NB 1 2 4, DROP, IO 0 1 2 exists
template <int NB, bool DROP = false, int IO = 0>
__global__ __launch_bounds__(TPB, NB > 2 ? 1 : 2) void k_fused_blk(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, 1, g.L, a.placement);
  const int b = w.b, d = w.dt * DT + 2 * j, rot = w.rot;
  const bool valid = d < g.D;
  const int dc = valid ? d : g.D - 2;
  RowBufT<IO> xb;
  if constexpr (IO == 0) xb = row_buf(a.in + (size_t)b * g.R * g.D, g, t, dc);
  else xb = row_buf<IO>(a.in, b, g, t, dc);
  LnLoad ln;
  ln.sb = a.ln_stats + (size_t)b * g.N;
  ln.g0 = a.ln_w ? a.ln_w[dc] : 1.f; ln.g1 = a.ln_w ? a.ln_w[dc + 1] : 1.f;
  ln.b0 = a.ln_b ? a.ln_b[dc] : 0.f; ln.b1 = a.ln_b ? a.ln_b[dc + 1] : 0.f;

  TState<NB> st;
  zero_acc<NB>(st);
  WPre wp;
  if constexpr (NB == 1) prefetch_w(wp, g, a.fa.w_re, a.fa.w_im, w.dt * DT, tid);
  forward_loop<NB, true>(st, lds, xb, a, t, j, 0, g.L, rot, &ln);
  unpack_filter<NB, 0, false>(st, lds, g, a.fa, b, d, valid, t, j, NB == 1 ? &wp : nullptr);
  __syncthreads();
  RowBufT<IO> yb;
  if constexpr (IO == 0) yb = row_buf(a.out + (size_t)b * g.R * g.D, g, t, d, valid);
  else yb = row_buf<IO>(a.out, b, g, t, d, valid);
  Drop dr{};
  if constexpr (DROP) dr = make_drop(a, b);
  inverse_loop<NB, true, DROP>(st, lds, yb, a, t, j, 0, g.L, rot, xb, dr, (unsigned)(dc >> 1));
  if constexpr (NB == 1) store_io<NB, 0>(st, g, a.fa, b, d, valid, t);
}

// ---- split path: (A) partial forward over a chunk of residues ---------------------------------
constexpr bool split_a_instance(int nb, bool drop, bool pad, int io) {
  return among<1, 2, 4>::has(nb) && among<0, 1, 2>::has(io) && !(pad && (drop || io != 0));
}
template <int NB, bool DROP = false, bool PAD = false, int IO = 0>
__global__ __launch_bounds__(TPB, 2) void k_split_a(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, a.nsplit, a.lc, a.placement);
  const int c = w.c, b = w.b, wg = b * ndt + w.dt, d = w.dt * DT + 2 * j;
  const bool valid = d < g.D;
  const int rbeg = c * a.lc, cnt = min(a.lc, g.L - rbeg);
  RowBufT<IO> xb;
  if constexpr (IO == 0) xb = row_buf(a.in + (size_t)b * g.R * g.D, g, t, valid ? d : g.D - 2);
  else xb = row_buf<IO>(a.in, b, g, t, valid ? d : g.D - 2);
  const int rot = w.rot % cnt;

  TState<NB> st;
  zero_acc<NB>(st);
  Drop dr{};
  if constexpr (DROP) dr = make_drop(a, b);
  forward_loop<NB, false, DROP, PAD>(st, lds, xb, a, t, j, rbeg, cnt, rot, nullptr, dr,
                                     (unsigned)((valid ? d : g.D - 2) >> 1));
  cf* z = a.ws_z + ((size_t)wg * a.nsplit + c) * (16 * NB * TPB);
#pragma unroll
  for (int sl = 0; sl < 16 * NB; ++sl) z[sl * TPB + tid] = st.acc[sl];
}

// (S) sum the nsplit partial spectra of every (b, d-tile): one block per (workgroup item, slot), so
// the whole chip takes part (a single CU streams only ~25 GB/s; with B*ndt blocks this step cost 25 us
// at C3).  Chunks are added in index order -> bitwise reproducible.
template <int NB>
__global__ __launch_bounds__(TPB) void k_split_sum(const DecimArgs a) {
  const int sl = blockIdx.x % (16 * NB), wg = blockIdx.x / (16 * NB), tid = threadIdx.x;
  const cf* z = a.ws_z + (size_t)wg * a.nsplit * (16 * NB * TPB) + sl * TPB + tid;
  cf acc = mk(0.f, 0.f);
  int c = 0;
  for (; c + 8 <= a.nsplit; c += 8) {
    cf v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = z[(size_t)(c + u) * (16 * NB * TPB)];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = cadd(acc, v[u]);
  }
  for (; c < a.nsplit; ++c) acc = cadd(acc, z[(size_t)c * (16 * NB * TPB)]);
  a.ws_zs[(size_t)wg * (16 * NB * TPB) + sl * TPB + tid] = acc;
}

// (F) unpack + filter the summed spectrum; emits S for (B) and the saved spectrum / grad slab
// (only B * ceil(D/32) < 384 workgroups exist on this plan, so one workgroup per CU costs nothing and
// lets the batched unpack of the multi-band variants keep its loads in registers instead of scratch)
template <int NB, int MODE>
__global__ __launch_bounds__(TPB, NB > 1 ? 1 : 2) void k_split_f(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const int wg = blockIdx.x, b = wg / ndt, d = (wg % ndt) * DT + 2 * j;
  const bool valid = d < g.D;
  TState<NB> st;
  // one band: this workgroup's 32-channel slice of (D, F) goes through LDS as in k_fused<1, .> (prefetch_w /
  // stage_w) -- no packed copy of the filter, no k_pack_w launch on the residue-split plan either
  WPre wp;
  constexpr bool STAGE_W = NB == 1 && MODE != 2;
  if constexpr (STAGE_W) prefetch_w(wp, g, a.fa.w_re, a.fa.w_im, (wg % ndt) * DT, tid);
  if (a.sum_in_f) {
    // the chunk partials of this (b, d-tile) summed here, in chunk order like k_split_sum (bitwise the same sums):
    // four slots x up to eight chunks = 32 loads in flight per thread.  One launch and one kernel boundary less per
    // direction; the 64 workgroups of C3 read 16.8 MB instead of 2.1, which costs less than the boundary did.
    const cf* z = a.ws_z + (size_t)wg * a.nsplit * (16 * NB * TPB) + tid;
    const size_t cs = (size_t)16 * NB * TPB;
#pragma unroll
    for (int s0 = 0; s0 < 16 * NB; s0 += 4) {
      cf sum[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) sum[i] = mk(0.f, 0.f);
      int c = 0;
      for (; c + 8 <= a.nsplit; c += 8) {
        cf v[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int u = 0; u < 8; ++u) v[i][u] = z[(size_t)(c + u) * cs + (s0 + i) * TPB];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int u = 0; u < 8; ++u) sum[i] = cadd(sum[i], v[i][u]);
      }
      for (; c < a.nsplit; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) sum[i] = cadd(sum[i], z[(size_t)c * cs + (s0 + i) * TPB]);
#pragma unroll
      for (int i = 0; i < 4; ++i) st.acc[s0 + i] = sum[i];
    }
  } else {
    const cf* z = a.ws_zs + (size_t)wg * (16 * NB * TPB);
#pragma unroll
    for (int sl = 0; sl < 16 * NB; ++sl) st.acc[sl] = z[sl * TPB + tid];
  }
  unpack_filter<NB, MODE, true>(st, lds, g, a.fa, b, d, valid, t, j, STAGE_W ? &wp : nullptr);
  if (a.ws_s == nullptr) return;
  cf* s = a.ws_s + (size_t)wg * (16 * NB * TPB);
#pragma unroll
  for (int sl = 0; sl < 16 * NB; ++sl) s[sl * TPB + tid] = st.acc[sl];
}

// (B) inverse over a chunk of residues, from the filtered spectrum parked by k_split_f / k_fused.
// (Folding the unpack + filter into this launch was measured: every chunk workgroup repeating the
// latency-bound prologue cost 33 us at C3, against 15 us for the separate B*ndt-block launch.)
constexpr bool split_b_instance(int nb, bool drop, bool acc, bool pad, int io) {
  if (!among<1, 2, 4>::has(nb) || !among<0, 1, 2>::has(io)) return false;
  if (acc) return nb == 4 && !drop && io == 0;
  return !(pad && (drop || io != 0));
}
template <int NB, bool DROP = false, bool ACC = false, bool PAD = false, int IO = 0>
__global__ __launch_bounds__(TPB, 2) void k_split_b(const DecimArgs a) {
  SMX_LDS_DECL;
  const Geom& g = a.g;
  const int tid = threadIdx.x, j = tid & 15, t = tid >> 4;
  const int ndt = (g.D + DT - 1) / DT;
  const WgItem w = wg_map(a.bid0 + blockIdx.x, g.B, ndt, a.nsplit, a.lc, a.placement);
  const int c = w.c, b = w.b, wg = b * ndt + w.dt, d = w.dt * DT + 2 * j;
  const bool valid = d < g.D;
  const int rbeg = c * a.lc, cnt = min(a.lc, g.L - rbeg);
  const int rot = w.rot % cnt;
  TState<NB> st;
  const cf* s = a.ws_s + (size_t)wg * (16 * NB * TPB);
#pragma unroll
  for (int sl = 0; sl < 16 * NB; ++sl) st.acc[sl] = s[sl * TPB + tid];
  RowBufT<IO> yb;
  if constexpr (IO == 0) yb = row_buf(a.out + (size_t)b * g.R * g.D, g, t, d, valid);
  else yb = row_buf<IO>(a.out, b, g, t, d, valid);
  Drop dr{};
  if constexpr (DROP) dr = make_drop(a, b);
  inverse_loop<NB, ACC, DROP, PAD>(st, lds, yb, a, t, j, rbeg, cnt, rot, yb, dr,
                                   (unsigned)((valid ? d : g.D - 2) >> 1));
}

// ---- launchers ---------------------------------------------------------------------------------
#ifdef SMX_MINI
// development only (never linked): the BASELINE kernels alone, for a quick look at their ISA --
//   hipcc --offload-arch=gfx950 -O3 ... --cuda-device-only -S -DSMX_MINI smx_decim.hip
template __global__ void k_fused<1, 0>(const DecimArgs);
template __global__ void k_fused<1, 1>(const DecimArgs);
template __global__ void k_fused<2, 0>(const DecimArgs);
template __global__ void k_fused<2, 1>(const DecimArgs);
template __global__ void k_split_a<1>(const DecimArgs);
template __global__ void k_split_b<1>(const DecimArgs);
template __global__ void k_split16_b<1>(const DecimArgs);
template __global__ void k_fused16<1, 0>(const DecimArgs);
#else
// Every launcher below: the template key from the arguments, the family's predicate (next to its kernel) asked once
// at run time -- no instance, no launch: hipErrorInvalidValue -- then pick_key under the same predicate and ONE launch
// statement.
static constexpr dim3 block_tpb() { return dim3(TPB); }

hipError_t launch_fused(const DecimArgs& a, int nb, int mode, hipStream_t s, int io, int oio) {
  const bool pad = a.g.R < a.g.N, acc = a.accumulate && a.out != nullptr;
  const bool drop = a.drop_thr != 0;     // mode 0: on the stored tile, mode 1: on the loaded tile
  if (oio < 0) oio = io;
  if (!fused_instance(nb, mode, drop, acc, pad, io, oio) || (io != 0 && a.accumulate))
    return hipErrorInvalidValue;         // (2-byte rows: no band groups)
  const int total = n_wg(a);
  return for_rounds(a, total, [&](const DecimArgs& r, dim3 grid) {
    pick_key([&](auto NB, auto MODE, auto DROP, auto ACC, auto PAD, auto IO, auto OIO) {
      if constexpr (fused_instance(SMX_KEY(NB), SMX_KEY(MODE), SMX_KEY(DROP), SMX_KEY(ACC), SMX_KEY(PAD), SMX_KEY(IO), SMX_KEY(OIO)))
        SMX_LAUNCH((k_fused<SMX_KEY(NB), SMX_KEY(MODE), SMX_KEY(DROP), SMX_KEY(ACC), SMX_KEY(PAD), SMX_KEY(IO), SMX_KEY(OIO)>), grid, block_tpb(), s, r);
      return true;
    }, among<1, 2, 4>{nb}, among<0, 1, 2>{mode}, flag{drop}, flag{acc}, flag{pad}, among<0, 1, 2>{io}, among<0, 1, 2>{oio});
  }, nb == 4);
}

hipError_t launch_fused16(const DecimArgs& a, int nb, int mode, hipStream_t s) {
  const bool pad = a.g.R < a.g.N, drop = a.drop_thr != 0 && mode != 2;      // (mode 2 stores and loads no rows to mask)
  if (!fused16_instance(nb, mode, pad, drop)) return hipErrorInvalidValue;
  return for_rounds(a, n_wg(a), [&](const DecimArgs& r, dim3 grid) {
    pick_key([&](auto NB, auto MODE, auto PAD, auto DROP) {
      if constexpr (fused16_instance(SMX_KEY(NB), SMX_KEY(MODE), SMX_KEY(PAD), SMX_KEY(DROP)))
        SMX_LAUNCH((k_fused16<SMX_KEY(NB), SMX_KEY(MODE), SMX_KEY(PAD), SMX_KEY(DROP)>), grid, block_tpb(), s, r);
      return true;
    }, among<1, 2>{nb}, among<0, 1, 2>{mode}, flag{pad}, flag{drop});
  });
}
// the split launches: drop = apply the dropout mask (A: to the loaded tile, B: to the stored tile)
hipError_t launch_split16_a(const DecimArgs& a, int nb, bool drop, hipStream_t s) {
  const bool pad = a.g.R < a.g.N, dr = drop && a.drop_thr != 0;
  if (!split16_instance(nb, pad, dr)) return hipErrorInvalidValue;
  return for_rounds(a, n_wg(a) * a.nsplit, [&](const DecimArgs& r, dim3 grid) {
    pick_key([&](auto NB, auto PAD, auto DROP) {
      if constexpr (split16_instance(SMX_KEY(NB), SMX_KEY(PAD), SMX_KEY(DROP)))
        SMX_LAUNCH((k_split16_a<SMX_KEY(NB), SMX_KEY(PAD), SMX_KEY(DROP)>), grid, block_tpb(), s, r);
      return true;
    }, among<1, 2>{nb}, flag{pad}, flag{dr});
  });
}
hipError_t launch_split16_b(const DecimArgs& a, int nb, bool drop, hipStream_t s) {
  const bool pad = a.g.R < a.g.N, dr = drop && a.drop_thr != 0;
  if (!split16_instance(nb, pad, dr)) return hipErrorInvalidValue;
  return for_rounds(a, n_wg(a) * a.nsplit, [&](const DecimArgs& r, dim3 grid) {
    pick_key([&](auto NB, auto PAD, auto DROP) {
      if constexpr (split16_instance(SMX_KEY(NB), SMX_KEY(PAD), SMX_KEY(DROP)))
        SMX_LAUNCH((k_split16_b<SMX_KEY(NB), SMX_KEY(PAD), SMX_KEY(DROP)>), grid, block_tpb(), s, r);
      return true;
    }, among<1, 2>{nb}, flag{pad}, flag{dr});
  });
}

hipError_t launch_synth(const DecimArgs& a, int nb, hipStream_t s) {
  if (!among<1, 2, 4>::has(nb)) return hipErrorInvalidValue;
  return for_rounds(a, n_wg(a), [&](const DecimArgs& r, dim3 grid) {
    pick_key([&](auto NB, auto PAD) {
      SMX_LAUNCH((k_synth<SMX_KEY(NB), SMX_KEY(PAD)>), grid, block_tpb(), s, r);
      return true;
    }, among<1, 2, 4>{nb}, flag{r.g.R < r.g.N});
  }, nb == 4);
}

hipError_t launch_synth8(const DecimArgs& a, hipStream_t s) {
  DecimArgs r = a;
  r.bid0 = 0;
  pick_bool(a.g.R < a.g.N, [&](auto PAD) {
    SMX_LAUNCH((k_synth8<SMX_KEY(PAD)>), dim3(n_wg(a)), block_tpb(), s, r);
    return true;
  });
  return launch_status();
}

hipError_t launch_full8(const DecimArgs& a, int mode, hipStream_t s) {
  DecimArgs r = a;
  r.bid0 = 0;
  const bool ok = pick_key([&](auto MODE, auto PAD) {
    SMX_LAUNCH((k_full8<SMX_KEY(MODE), SMX_KEY(PAD)>), dim3(n_wg(a)), block_tpb(), s, r);
    return true;
  }, among<0, 1, 2>{mode}, flag{a.g.R < a.g.N});
  return ok ? launch_status() : hipErrorInvalidValue;
}

hipError_t launch_fused_block(const DecimArgs& a, int nb, hipStream_t s, int io) {
  const bool drop = a.drop_thr != 0;
  // (the kernel serves neither zero-padded rows nor accumulating band groups; the block plan has neither)
  if (a.g.R < a.g.N || a.accumulate || !among<1, 2, 4>::has(nb) || !among<0, 1, 2>::has(io)) return hipErrorInvalidValue;
  return for_rounds(a, n_wg(a), [&](const DecimArgs& r, dim3 grid) {
    pick_key([&](auto NB, auto DROP, auto IO) {
      SMX_LAUNCH((k_fused_blk<SMX_KEY(NB), SMX_KEY(DROP), SMX_KEY(IO)>), grid, block_tpb(), s, r);
      return true;
    }, among<1, 2, 4>{nb}, flag{drop}, among<0, 1, 2>{io});
  }, nb == 4);
}

hipError_t launch_split_a(const DecimArgs& a, int nb, bool drop_in, hipStream_t s, int io) {
  const bool pad = a.g.R < a.g.N, drop = drop_in && a.drop_thr != 0;
  if (!split_a_instance(nb, drop, pad, io) || (io != 0 && a.accumulate)) return hipErrorInvalidValue;
  return for_rounds(a, n_wg(a) * a.nsplit, [&](const DecimArgs& r, dim3 grid) {
    pick_key([&](auto NB, auto DROP, auto PAD, auto IO) {
      if constexpr (split_a_instance(SMX_KEY(NB), SMX_KEY(DROP), SMX_KEY(PAD), SMX_KEY(IO)))
        SMX_LAUNCH((k_split_a<SMX_KEY(NB), SMX_KEY(DROP), SMX_KEY(PAD), SMX_KEY(IO)>), grid, block_tpb(), s, r);
      return true;
    }, among<1, 2, 4>{nb}, flag{drop}, flag{pad}, among<0, 1, 2>{io});
  });
}

hipError_t launch_split_f(const DecimArgs& a, int nb, int mode, hipStream_t s) {
  if (!among<1, 2, 4>::has(nb) || !among<0, 1, 2>::has(mode)) return hipErrorInvalidValue;
  if (!a.sum_in_f)
    pick<1, 2, 4>(nb, [&](auto NB) {
      SMX_LAUNCH((k_split_sum<SMX_KEY(NB)>), dim3(n_wg(a) * 16 * nb), block_tpb(), s, a);
      return true;
    });
  pick_key([&](auto NB, auto MODE) {
    SMX_LAUNCH((k_split_f<SMX_KEY(NB), SMX_KEY(MODE)>), dim3(n_wg(a)), block_tpb(), s, a);
    return true;
  }, among<1, 2, 4>{nb}, among<0, 1, 2>{mode});
  return launch_status();
}

hipError_t launch_split_b(const DecimArgs& a, int nb, bool drop_out, hipStream_t s, int io) {
  const bool pad = a.g.R < a.g.N, acc = a.accumulate != 0, drop = drop_out && a.drop_thr != 0;
  if (!split_b_instance(nb, drop, acc, pad, io)) return hipErrorInvalidValue;
  return for_rounds(a, n_wg(a) * a.nsplit, [&](const DecimArgs& r, dim3 grid) {
    pick_key([&](auto NB, auto DROP, auto ACC, auto PAD, auto IO) {
      if constexpr (split_b_instance(SMX_KEY(NB), SMX_KEY(DROP), SMX_KEY(ACC), SMX_KEY(PAD), SMX_KEY(IO)))
        SMX_LAUNCH((k_split_b<SMX_KEY(NB), SMX_KEY(DROP), SMX_KEY(ACC), SMX_KEY(PAD), SMX_KEY(IO)>), grid, block_tpb(), s, r);
      return true;
    }, among<1, 2, 4>{nb}, flag{drop}, flag{acc}, flag{pad}, among<0, 1, 2>{io});
  });
}

#endif  // SMX_MINI

}  // namespace smx
