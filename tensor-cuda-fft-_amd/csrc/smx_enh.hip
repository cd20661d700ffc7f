// smx_enh.hip -- row kernels of EnhancedSpectralBlock (reference fft_tensor/spectral_enhancements.py:278-333):
//     x1 = x  + drop(rope(norm1(x)))          A: k_rope_fwd / k_rope_bwd   (+ norm2(x1) for the next line)
//     x2 = x1 + drop(phase_mixing(h2))        B: k_res_fwd / k_res_bwd     (+ norm3(x2))
//     x3 = x2 + drop(gated(h3))               C: k_gate_fwd / k_gate_bwd   (gate_proj's LayerNorm over 2D,
//                                                 sigmoid gate, blend, residual; the two Linears stay GEMMs)
// The transforms of phase_mixing / multi_scale and the GEMMs run elsewhere; what is here is the row work torch
// would do in many small passes.  One wavefront per (b, t) row, lane l holds elements (l + 64 c) VEC + [0, VEC),
// c < CH, in registers; the row helpers, the LayerNorm-backward step and the launch are smx_rows.h's; every global access is a full-wave contiguous segment, every row is read
// once and written once.  Dropout uses the library's counter-based mask (smx_core.h, Drop): element t D + d of
// batch row b, so the backward regenerates the forward's mask from the same two words.  LayerNorm parameter
// gradients are per-workgroup partials reduced by k_ln_colsum in a fixed order (no atomics: bitwise reproducible).
#include "smx_kernels.h"
#include "smx_rows.h"

namespace smx {

namespace {

// ---- A: rope line.  NORM = false is the standalone RotaryFrequencyEmbedding: out = rot(x) ------------------------
// rot: row t of the (max_seq_len, D/2) complex64 table, D floats (cos, sin) in the layout of a row of x.
template <int VEC, int CH, bool NORM>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_rope_fwd(const float* __restrict__ x, const float* __restrict__ rot,
                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      float eps1, float eps2, float* __restrict__ x1,
                                                      float* __restrict__ h2, cf* __restrict__ stats, long long rows,
                                                      int T, int D, unsigned thr, float scale,
                                                      const unsigned long long* __restrict__ rng) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  Vec<VEC> gm1[CH], bt1[CH], gm2[CH], bt2[CH];
  if (NORM) {
    row_load_cached(gm1, w1, D, lane, 1.f); row_load_cached(bt1, b1, D, lane, 0.f);
    row_load_cached(gm2, w2, D, lane, 1.f); row_load_cached(bt2, b2, D, lane, 0.f);
  }
  const unsigned long long s0 = thr ? rng[0] : 0ull, s1 = thr ? rng[1] : 0ull;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows; row += (long long)gridDim.x * ROW_WAVES) {
    const int t = (int)(row % T), b = (int)(row / T);
    const size_t o = (size_t)row * D;
    Vec<VEC> xv[CH], h[CH], rv[CH];
    row_load(xv, x + o, D, lane);
    row_load_cached(rv, rot + (size_t)t * D, D, lane, 0.f);
    cf st1 = mk(0.f, 1.f);
    if (NORM) st1 = row_stats(xv, D, lane, eps1);
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int i = 0; i < VEC; i += 2) {
        float a0 = xv[c].v[i], a1 = xv[c].v[i + 1];
        if (NORM) {
          a0 = fmaf((a0 - st1.x) * st1.y, gm1[c].v[i], bt1[c].v[i]);
          a1 = fmaf((a1 - st1.x) * st1.y, gm1[c].v[i + 1], bt1[c].v[i + 1]);
        }
        const float cs = rv[c].v[i], sn = rv[c].v[i + 1];
        h[c].v[i] = a0 * cs - a1 * sn;
        h[c].v[i + 1] = a0 * sn + a1 * cs;
      }
    if (!NORM) {
      row_store(h, x1 + o, D, lane);
      continue;
    }
    const unsigned key = thr ? drop_row_key(s0, s1, b) : 0u;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float m[VEC];
      if (thr) drop_factors<VEC>(m, key, (unsigned long long)t * D + (lane + 64 * c) * VEC, thr, scale);
#pragma unroll
      for (int i = 0; i < VEC; ++i) xv[c].v[i] = thr ? fmaf(m[i], h[c].v[i], xv[c].v[i]) : xv[c].v[i] + h[c].v[i];
    }
    const cf st2 = row_stats(xv, D, lane, eps2);
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) h[c].v[i] = fmaf((xv[c].v[i] - st2.x) * st2.y, gm2[c].v[i], bt2[c].v[i]);
    row_store(xv, x1 + o, D, lane);
    row_store(h, h2 + o, D, lane);
    if (lane == 0) { stats[row] = st1; stats[rows + row] = st2; }
  }
}

// Backward of A given g1 = dL/dx1 and gh2 = dL/dh2:  G = g1 + LN2'(gh2),  gh1 = rot^T(M1 G),  grad_x = G + LN1'(gh1),
// x1 recomputed from x in registers.  NORM = false: grad_x = rot^T(g1).
template <int VEC, int CH, bool NORM>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_rope_bwd(const float* __restrict__ g1, const float* __restrict__ gh2,
                                                      const float* __restrict__ x, const float* __restrict__ rot,
                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const cf* __restrict__ stats,
                                                      float* __restrict__ gx, float* __restrict__ part,
                                                      long long rows, int T, int D, unsigned thr, float scale,
                                                      const unsigned long long* __restrict__ rng) {
  __shared__ float red[NORM ? ROW_WAVES : 1][2][64 * VEC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_d = 1.f / (float)D;
  Vec<VEC> gm1[CH], bt1[CH], gm2[CH], ag1[CH], ab1[CH], ag2[CH], ab2[CH];
  if (NORM) {
    row_load_cached(gm1, w1, D, lane, 1.f); row_load_cached(bt1, b1, D, lane, 0.f);
    row_load_cached(gm2, w2, D, lane, 1.f);
    zero(ag1); zero(ab1); zero(ag2); zero(ab2);
  }
  const unsigned long long s0 = thr ? rng[0] : 0ull, s1 = thr ? rng[1] : 0ull;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows; row += (long long)gridDim.x * ROW_WAVES) {
    const int t = (int)(row % T), b = (int)(row / T);
    const size_t o = (size_t)row * D;
    Vec<VEC> G[CH], rv[CH], xh1[CH];
    row_load(G, g1 + o, D, lane);
    row_load_cached(rv, rot + (size_t)t * D, D, lane, 0.f);
    const unsigned key = (NORM && thr) ? drop_row_key(s0, s1, b) : 0u;
    cf st1 = mk(0.f, 1.f);
    if (NORM) {
      st1 = stats[row];
      const cf st2 = stats[rows + row];
      Vec<VEC> xh2[CH], u[CH];
      row_load(xh1, x + o, D, lane);
      row_load(u, gh2 + o, D, lane);
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int e = (lane + 64 * c) * VEC;
        float m[VEC];
        if (thr) drop_factors<VEC>(m, key, (unsigned long long)t * D + e, thr, scale);
#pragma unroll
        for (int i = 0; i < VEC; i += 2) {
          const float xa = xh1[c].v[i], xb = xh1[c].v[i + 1];
          const float na = (xa - st1.x) * st1.y, nb = (xb - st1.x) * st1.y;
          const float a0 = fmaf(na, gm1[c].v[i], bt1[c].v[i]), a1 = fmaf(nb, gm1[c].v[i + 1], bt1[c].v[i + 1]);
          const float cs = rv[c].v[i], sn = rv[c].v[i + 1];
          const float r0 = a0 * cs - a1 * sn, r1 = a0 * sn + a1 * cs;
          const float y0 = thr ? fmaf(m[i], r0, xa) : xa + r0, y1 = thr ? fmaf(m[i + 1], r1, xb) : xb + r1;
          xh1[c].v[i] = e < D ? na : 0.f;
          xh1[c].v[i + 1] = e < D ? nb : 0.f;
          xh2[c].v[i] = e < D ? (y0 - st2.x) * st2.y : 0.f;
          xh2[c].v[i + 1] = e < D ? (y1 - st2.x) * st2.y : 0.f;
        }
        // ln_bwd_acc / ln_bwd_apply written out: inside this chunk loop they changed which product of the
        // rotation below is fused into an fma in k_rope_bwd<2, 1, true>
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float gh = u[c].v[i];
          ag2[c].v[i] = fmaf(gh, xh2[c].v[i], ag2[c].v[i]);
          ab2[c].v[i] += gh;
          const float uu = gm2[c].v[i] * gh;
          u[c].v[i] = uu;
          s1 += uu;
          s2 = fmaf(uu, xh2[c].v[i], s2);
        }
      }
      const float m1 = wave_sum(s1) * inv_d, m2 = wave_sum(s2) * inv_d;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int i = 0; i < VEC; ++i) G[c].v[i] = fmaf(st2.y, u[c].v[i] - m1 - xh2[c].v[i] * m2, G[c].v[i]);
    }
    // gh1 = rot^T(M1 G): rotation by the conjugate
    Vec<VEC> gh[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float m[VEC];
      if (NORM && thr) drop_factors<VEC>(m, key, (unsigned long long)t * D + (lane + 64 * c) * VEC, thr, scale);
#pragma unroll
      for (int i = 0; i < VEC; i += 2) {
        float a = G[c].v[i], bb = G[c].v[i + 1];
        if (NORM && thr) { a *= m[i]; bb *= m[i + 1]; }
        const float cs = rv[c].v[i], sn = rv[c].v[i + 1];
        gh[c].v[i] = a * cs + bb * sn;
        gh[c].v[i + 1] = bb * cs - a * sn;
      }
    }
    if (!NORM) {
      row_store(gh, gx + o, D, lane);
      continue;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        gh[c].v[i] = ln_bwd_acc(gh[c].v[i], xh1[c].v[i], gm1[c].v[i], ag1[c].v[i], ab1[c].v[i], s1, s2);
    ln_bwd_apply(G, gh, xh1, st1.y, wave_sum(s1) * inv_d, wave_sum(s2) * inv_d);
    row_store(G, gx + o, D, lane);
  }
  if (NORM) {
    const size_t nblk = gridDim.x;
    block_partials(ag1, ab1, part + (size_t)blockIdx.x * 2 * D, D, 0, D, red, lane, wv);
    block_partials(ag2, ab2, part + (nblk + blockIdx.x) * 2 * D, D, 0, D, red, lane, wv);
  }
}

// ---- B: x2 = x1 + M2 p,  h3 = LN(x2) ----------------------------------------------------------------------------
template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_res_fwd(const float* __restrict__ x1, const float* __restrict__ p,
                                                     const float* __restrict__ w3, const float* __restrict__ b3,
                                                     float eps, float* __restrict__ x2, float* __restrict__ h3,
                                                     cf* __restrict__ stats, long long rows, int T, int D,
                                                     unsigned thr, float scale,
                                                     const unsigned long long* __restrict__ rng) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  Vec<VEC> gm[CH], bt[CH];
  row_load_cached(gm, w3, D, lane, 1.f); row_load_cached(bt, b3, D, lane, 0.f);
  const unsigned long long s0 = thr ? rng[0] : 0ull, s1 = thr ? rng[1] : 0ull;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows; row += (long long)gridDim.x * ROW_WAVES) {
    const int t = (int)(row % T), b = (int)(row / T);
    const size_t o = (size_t)row * D;
    Vec<VEC> xv[CH], pv[CH];
    row_load(xv, x1 + o, D, lane);
    row_load(pv, p + o, D, lane);
    const unsigned key = thr ? drop_row_key(s0, s1, b) : 0u;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float m[VEC];
      if (thr) drop_factors<VEC>(m, key, (unsigned long long)t * D + (lane + 64 * c) * VEC, thr, scale);
#pragma unroll
      for (int i = 0; i < VEC; ++i) xv[c].v[i] = thr ? fmaf(m[i], pv[c].v[i], xv[c].v[i]) : xv[c].v[i] + pv[c].v[i];
    }
    const cf st = row_stats(xv, D, lane, eps);
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) pv[c].v[i] = fmaf((xv[c].v[i] - st.x) * st.y, gm[c].v[i], bt[c].v[i]);
    row_store(xv, x2 + o, D, lane);
    row_store(pv, h3 + o, D, lane);
    if (lane == 0) stats[row] = st;
  }
}

// G = g2 + LN3'(gh3):  grad_x1 = G,  grad_p = M2 G (not written when gp == NULL)
template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_res_bwd(const float* __restrict__ g2, const float* __restrict__ gh3,
                                                     const float* __restrict__ x2, const float* __restrict__ w3,
                                                     const cf* __restrict__ stats, float* __restrict__ gx1,
                                                     float* __restrict__ gp, float* __restrict__ part, long long rows,
                                                     int T, int D, unsigned thr, float scale,
                                                     const unsigned long long* __restrict__ rng) {
  __shared__ float red[ROW_WAVES][2][64 * VEC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_d = 1.f / (float)D;
  Vec<VEC> gm[CH], ag[CH], ab[CH];
  row_load_cached(gm, w3, D, lane, 1.f);
  zero(ag); zero(ab);
  const unsigned long long s0 = thr ? rng[0] : 0ull, s1 = thr ? rng[1] : 0ull;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows; row += (long long)gridDim.x * ROW_WAVES) {
    const int t = (int)(row % T), b = (int)(row / T);
    const size_t o = (size_t)row * D;
    Vec<VEC> G[CH], xh[CH], u[CH];
    row_load(G, g2 + o, D, lane);
    row_load(xh, x2 + o, D, lane);
    row_load(u, gh3 + o, D, lane);
    const cf st = stats[row];
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        xh[c].v[i] = e < D ? (xh[c].v[i] - st.x) * st.y : 0.f;
        u[c].v[i] = ln_bwd_acc(u[c].v[i], xh[c].v[i], gm[c].v[i], ag[c].v[i], ab[c].v[i], sa, sb);
      }
    }
    ln_bwd_apply(G, u, xh, st.y, wave_sum(sa) * inv_d, wave_sum(sb) * inv_d);
    row_store(G, gx1 + o, D, lane);
    if (gp) {
      const unsigned key = thr ? drop_row_key(s0, s1, b) : 0u;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        float m[VEC];
        if (thr) drop_factors<VEC>(m, key, (unsigned long long)t * D + (lane + 64 * c) * VEC, thr, scale);
#pragma unroll
        for (int i = 0; i < VEC; ++i) G[c].v[i] *= thr ? m[i] : 1.f;
      }
      row_store(G, gp + o, D, lane);
    }
  }
  block_partials(ag, ab, part + (size_t)blockIdx.x * 2 * D, D, 0, D, red, lane, wv);
}

// ---- C: a (rows, 2D) = gate_proj[0](h3), v (rows, D) = value_proj(h3):
//   â = LN_2D(a),  gate = sigmoid(â[:D]),  out = gate v + (1 - gate) â[D:],  x3 = x2 + M3 out  (x2 == NULL: x3 = out)
template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_gate_fwd(const float* __restrict__ a, const float* __restrict__ v,
                                                      const float* __restrict__ x2, const float* __restrict__ wg,
                                                      const float* __restrict__ bg, float eps,
                                                      float* __restrict__ x3, cf* __restrict__ stats, long long rows,
                                                      int T, int D, unsigned thr, float scale,
                                                      const unsigned long long* __restrict__ rng) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_w = 0.5f / (float)D;
  Vec<VEC> gl[CH], gh[CH], bl[CH], bh[CH];
  row_load_cached(gl, wg, D, lane, 1.f); row_load_cached(gh, wg ? wg + D : nullptr, D, lane, 1.f);
  row_load_cached(bl, bg, D, lane, 0.f); row_load_cached(bh, bg ? bg + D : nullptr, D, lane, 0.f);
  const unsigned long long s0 = thr ? rng[0] : 0ull, s1 = thr ? rng[1] : 0ull;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows; row += (long long)gridDim.x * ROW_WAVES) {
    const int t = (int)(row % T), b = (int)(row / T);
    const size_t o = (size_t)row * D;
    Vec<VEC> al[CH], ah[CH], vv[CH], rv[CH];
    row_load(al, a + 2 * o, D, lane);
    row_load(ah, a + 2 * o + D, D, lane);
    row_load(vv, v + o, D, lane);
    if (x2) row_load(rv, x2 + o, D, lane);
    else zero(rv);
    const float mean = wave_sum(row_sum(al) + row_sum(ah)) * inv_w;
    const float var = wave_sum(row_sq(al, mean, D, lane) + row_sq(ah, mean, D, lane)) * inv_w;
    const cf st = mk(mean, 1.f / sqrtf(var + eps));
    const unsigned key = thr ? drop_row_key(s0, s1, b) : 0u;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float m[VEC];
      if (thr) drop_factors<VEC>(m, key, (unsigned long long)t * D + (lane + 64 * c) * VEC, thr, scale);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float zg = fmaf((al[c].v[i] - st.x) * st.y, gl[c].v[i], bl[c].v[i]);
        const float vt = fmaf((ah[c].v[i] - st.x) * st.y, gh[c].v[i], bh[c].v[i]);
        const float gate = 1.f / (1.f + expf(-zg));
        const float out = gate * vv[c].v[i] + (1.f - gate) * vt;
        rv[c].v[i] = thr ? fmaf(m[i], out, rv[c].v[i]) : rv[c].v[i] + out;
      }
    }
    row_store(rv, x3 + o, D, lane);
    if (lane == 0) stats[row] = st;
  }
}

// go = M3 g3:  grad_v = gate go,  gâ[:D] = go (v - vt) gate (1 - gate),  gâ[D:] = go (1 - gate),  grad_a = LN_2D'(gâ)
template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_gate_bwd(const float* __restrict__ g3, const float* __restrict__ a,
                                                      const float* __restrict__ v, const float* __restrict__ wg,
                                                      const float* __restrict__ bg, const cf* __restrict__ stats,
                                                      float* __restrict__ ga, float* __restrict__ gv,
                                                      float* __restrict__ part, long long rows, int T, int D,
                                                      unsigned thr, float scale,
                                                      const unsigned long long* __restrict__ rng) {
  __shared__ float red[ROW_WAVES][2][64 * VEC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_w = 0.5f / (float)D;
  Vec<VEC> gl[CH], gh[CH], bl[CH], bh[CH], agl[CH], agh[CH], abl[CH], abh[CH];
  row_load_cached(gl, wg, D, lane, 1.f); row_load_cached(gh, wg ? wg + D : nullptr, D, lane, 1.f);
  row_load_cached(bl, bg, D, lane, 0.f); row_load_cached(bh, bg ? bg + D : nullptr, D, lane, 0.f);
  zero(agl); zero(agh); zero(abl); zero(abh);
  const unsigned long long s0 = thr ? rng[0] : 0ull, s1 = thr ? rng[1] : 0ull;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows; row += (long long)gridDim.x * ROW_WAVES) {
    const int t = (int)(row % T), b = (int)(row / T);
    const size_t o = (size_t)row * D;
    // al / ah: the row of a, then its normalised halves;  ul / vv: the row of g3 / v, then gamma * dL/dâ of each half
    Vec<VEC> al[CH], ah[CH], vv[CH], ul[CH];
    row_load(ul, g3 + o, D, lane);
    row_load(al, a + 2 * o, D, lane);
    row_load(ah, a + 2 * o + D, D, lane);
    row_load(vv, v + o, D, lane);
    const cf st = stats[row];
    const unsigned key = thr ? drop_row_key(s0, s1, b) : 0u;
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      float m[VEC];
      if (thr) drop_factors<VEC>(m, key, (unsigned long long)t * D + e, thr, scale);
      Vec<VEC> gvv;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float g = thr ? ul[c].v[i] * m[i] : ul[c].v[i];
        const float nl = e < D ? (al[c].v[i] - st.x) * st.y : 0.f;
        const float nh = e < D ? (ah[c].v[i] - st.x) * st.y : 0.f;
        const float zg = fmaf(nl, gl[c].v[i], bl[c].v[i]);
        const float vt = fmaf(nh, gh[c].v[i], bh[c].v[i]);
        const float gate = 1.f / (1.f + expf(-zg));
        const float dl = g * (vv[c].v[i] - vt) * gate * (1.f - gate);
        const float dh = g * (1.f - gate);
        gvv.v[i] = gate * g;
        agl[c].v[i] = fmaf(dl, nl, agl[c].v[i]);
        agh[c].v[i] = fmaf(dh, nh, agh[c].v[i]);
        abl[c].v[i] += dl;
        abh[c].v[i] += dh;
        // the LayerNorm-backward step over a 2D-wide row held as two halves: both halves feed one pair of sums
        // and nothing is added to the result, so ln_bwd_acc / ln_bwd_apply (smx_rows.h) do not fit
        const float u0 = gl[c].v[i] * dl, u1 = gh[c].v[i] * dh;
        sa += u0 + u1;
        sb = fmaf(u0, nl, fmaf(u1, nh, sb));
        al[c].v[i] = nl; ah[c].v[i] = nh;
        ul[c].v[i] = u0; vv[c].v[i] = u1;
      }
      if (e < D) gvv.store(gv + o + e);
    }
    const float m1 = wave_sum(sa) * inv_w, m2 = wave_sum(sb) * inv_w;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        ul[c].v[i] = st.y * (ul[c].v[i] - m1 - al[c].v[i] * m2);
        vv[c].v[i] = st.y * (vv[c].v[i] - m1 - ah[c].v[i] * m2);
      }
    row_store(ul, ga + 2 * o, D, lane);
    row_store(vv, ga + 2 * o + D, D, lane);
  }
  float* pb = part + (size_t)blockIdx.x * 4 * D;          // this block's (2, 2D) slab
  block_partials(agl, abl, pb, 2 * D, 0, D, red, lane, wv);
  block_partials(agh, abh, pb, 2 * D, D, D, red, lane, wv);
}

// (VEC, CH) of a D-wide row (even, <= ENH_MAX_D): Vec<4> tiles up to 4 chunks when D % 4 == 0, else Vec<2> up to 8
template <typename Fn>
bool enh_dispatch(int D, Fn f) {
  return D % 4 == 0 ? row_dispatch<4, 4>(D, f) : row_dispatch<2, 8>(D, f);
}

}  // namespace

bool enh_supported(int D) { return D >= 2 && D % 2 == 0 && D <= ENH_MAX_D; }

size_t enh_part_floats(long long rows, int D) { return (size_t)ln_num_blocks(rows) * 4 * (size_t)D; }

hipError_t launch_rope_fwd(const float* x, const float* rot, const float* w1, const float* b1, const float* w2,
                           const float* b2, float eps1, float eps2, float* x1, float* h2, cf* stats, int B, int T,
                           int D, bool norm, unsigned thr, float scale, const unsigned long long* rng, hipStream_t s) {
  const long long rows = (long long)B * T;
  enh_dispatch(D, [&](auto vec, auto ch) {
    constexpr int V = decltype(vec)::value, C = decltype(ch)::value;
    if (norm)
      row_launch(k_rope_fwd<V, C, true>, rows, s, x, rot, w1, b1, w2, b2, eps1, eps2, x1, h2,
                         stats, rows, T, D, thr, scale, rng);
    else
      row_launch(k_rope_fwd<V, C, false>, rows, s, x, rot, w1, b1, w2, b2, eps1, eps2, x1, h2,
                         stats, rows, T, D, 0u, 1.f, rng);
  });
  return hipGetLastError();
}

hipError_t launch_rope_bwd(const float* g1, const float* gh2, const float* x, const float* rot, const float* w1,
                           const float* b1, const float* w2, const cf* stats, float* gx, float* gw1, float* gb1,
                           float* gw2, float* gb2, float* part, int B, int T, int D, bool norm, unsigned thr,
                           float scale, const unsigned long long* rng, hipStream_t s) {
  const long long rows = (long long)B * T;
  const int nblk = ln_num_blocks(rows);
  enh_dispatch(D, [&](auto vec, auto ch) {
    constexpr int V = decltype(vec)::value, C = decltype(ch)::value;
    if (norm)
      row_launch(k_rope_bwd<V, C, true>, rows, s, g1, gh2, x, rot, w1, b1, w2, stats, gx, part,
                         rows, T, D, thr, scale, rng);
    else
      row_launch(k_rope_bwd<V, C, false>, rows, s, g1, gh2, x, rot, w1, b1, w2, stats, gx, part,
                         rows, T, D, 0u, 1.f, rng);
  });
  if (hipError_t e = hipGetLastError()) return e;
  if (!norm) return hipSuccess;
  if (hipError_t e = launch_ln_colsum(part, nblk, D, gw1, gb1, s)) return e;
  return launch_ln_colsum(part + (size_t)nblk * 2 * D, nblk, D, gw2, gb2, s);
}

hipError_t launch_res_fwd(const float* x1, const float* p, const float* w3, const float* b3, float eps, float* x2,
                          float* h3, cf* stats, int B, int T, int D, unsigned thr, float scale,
                          const unsigned long long* rng, hipStream_t s) {
  const long long rows = (long long)B * T;
  enh_dispatch(D, [&](auto vec, auto ch) {
    row_launch(k_res_fwd<decltype(vec)::value, decltype(ch)::value>, rows, s, x1, p, w3, b3, eps,
                       x2, h3, stats, rows, T, D, thr, scale, rng);
  });
  return hipGetLastError();
}

hipError_t launch_res_bwd(const float* g2, const float* gh3, const float* x2, const float* w3, const cf* stats,
                          float* gx1, float* gp, float* gw3, float* gb3, float* part, int B, int T, int D, unsigned thr,
                          float scale, const unsigned long long* rng, hipStream_t s) {
  const long long rows = (long long)B * T;
  const int nblk = ln_num_blocks(rows);
  enh_dispatch(D, [&](auto vec, auto ch) {
    row_launch(k_res_bwd<decltype(vec)::value, decltype(ch)::value>, rows, s, g2, gh3, x2, w3,
                       stats, gx1, gp, part, rows, T, D, thr, scale, rng);
  });
  if (hipError_t e = hipGetLastError()) return e;
  return launch_ln_colsum(part, nblk, D, gw3, gb3, s);
}

hipError_t launch_gate_blend_fwd(const float* a, const float* v, const float* x2, const float* wg, const float* bg,
                                 float eps, float* x3, cf* stats, int B, int T, int D, unsigned thr, float scale,
                                 const unsigned long long* rng, hipStream_t s) {
  const long long rows = (long long)B * T;
  enh_dispatch(D, [&](auto vec, auto ch) {
    row_launch(k_gate_fwd<decltype(vec)::value, decltype(ch)::value>, rows, s, a, v, x2, wg, bg,
                       eps, x3, stats, rows, T, D, thr, scale, rng);
  });
  return hipGetLastError();
}

hipError_t launch_gate_blend_bwd(const float* g3, const float* a, const float* v, const float* wg, const float* bg,
                                 const cf* stats, float* ga, float* gv, float* gwg, float* gbg, float* part, int B,
                                 int T, int D, unsigned thr, float scale, const unsigned long long* rng,
                                 hipStream_t s) {
  const long long rows = (long long)B * T;
  const int nblk = ln_num_blocks(rows);
  enh_dispatch(D, [&](auto vec, auto ch) {
    row_launch(k_gate_bwd<decltype(vec)::value, decltype(ch)::value>, rows, s, g3, a, v, wg, bg,
                       stats, ga, gv, part, rows, T, D, thr, scale, rng);
  });
  if (hipError_t e = hipGetLastError()) return e;
  return launch_ln_colsum(part, nblk, 2 * D, gwg, gbg, s);
}

}  // namespace smx
