// smx_block.hip -- row kernels of the fused SpectralMLPBlock first half:
//     y = x + SpectralMixingLayer(LayerNorm(x))          reference fft_tensor/spectral_layers.py:185
//
// The LayerNorm itself is folded into the load of the decimated forward kernel and the residual add
// into its store (smx_decim.hip, k_fused_blk); what remains here is
//   * k_ln_stats    per-row (mean, rstd): the one extra read of x the fusion cannot avoid -- a row's
//                   statistics need all D channels, a workgroup of the transform owns 32;
//   * k_ln_bwd      LayerNorm backward + residual: grad_x = g + LN'(grad_h), in place over grad_h, and
//                   the per-block partial sums of grad_gamma / grad_beta;
//                   (2-byte rows, IO != 0: grad_h stays f32 in a scratch of its own, x / g are read and grad_x is
//                   written in the IO type -- not in place, the same arithmetic, one rounding at the store);
//   * k_ln_colsum   fixed-order reduction of those partials (bitwise reproducible);
//   * k_ln_apply, k_add_rows   unfused fallback used with the split / direct transform paths;
//   * k_head_fwd, k_head_bwd   the 1- or 2-neuron head of fft_lm's word-structure models over all B T rows: the same row
//                   walk, its parameter-gradient partials in the slab layout k_ln_colsum reduces;
//   * k_xent_fwd, k_xent_bwd   softmax cross-entropy over rows of logits of a LayerNorm row width, the same row walk;
//     k_xent_fwd_stream, k_xent_bwd_stream   the same for any wider row (the 50257-way token loss of fft_lm's dual head):
//                   one workgroup per row, a running (max, sum) per thread; k_xent_finish adds the per-block (sum, count)
//                   partials of either in a fixed order.
// One wavefront per row, lane l holds elements (l + 64 c) VEC + [0, VEC), c < CH, in registers:
// every global access is a full-wave contiguous segment and a row is read exactly once.
// Vec, wave_sum, the LayerNorm-backward accumulation, the (VEC, CH) dispatch and the launch geometry
// (ROW_WAVES rows per block, ln_num_blocks blocks) are smx_rows.h's.  The load, statistics and partial
// loops of the three kernels stay written out: each fuses what the toolkit keeps apart (two rows in
// flight, one bounds test for three loads, the update fused with its store, 64-bit slab offsets), and
// every helper spelling tried compiled to other registers.
#include "smx_kernels.h"
#include "smx_rows.h"

namespace smx {

namespace {

// stats[row] = (mean, 1/sqrt(var + eps)), biased variance, two passes over the registers
// (torch.nn.LayerNorm, used by the reference at spectral_layers.py:162,185).
// IO: element type of x (smx_rows.h io_elem); the statistics are f32 whatever it is.
template <int VEC, int CH, int IO = 0>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_ln_stats(const io_elem<IO>* __restrict__ x,
                                                             cf* __restrict__ stats, long long rows,
                                                             int D, float eps) {
  constexpr int R = CH <= 2 ? 2 : 1;          // rows in flight per wavefront (read-only kernel)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_d = 1.f / (float)D;
  const long long step = (long long)gridDim.x * ROW_WAVES;
  for (long long row0 = (long long)blockIdx.x * ROW_WAVES + wv; row0 < rows; row0 += R * step) {
    Vec<VEC> xv[R][CH];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const long long row = row0 + q * step;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int e = (lane + 64 * c) * VEC;
        if (e < D && row < rows) load_io<IO>(xv[q][c], x + (size_t)row * D + e);
        else
#pragma unroll
          for (int i = 0; i < VEC; ++i) xv[q][c].v[i] = 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const long long row = row0 + q * step;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int i = 0; i < VEC; ++i) s += xv[q][c].v[i];
      const float mean = wave_sum(s) * inv_d;
      float v2 = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int e = (lane + 64 * c) * VEC;
        if (e < D)
#pragma unroll
          for (int i = 0; i < VEC; ++i) { const float dl = xv[q][c].v[i] - mean; v2 = fmaf(dl, dl, v2); }
      }
      const float var = wave_sum(v2) * inv_d;
      if (lane == 0 && row < rows) stats[row] = mk(mean, 1.f / sqrtf(var + eps));
    }
  }
}

// h = (x - mean) rstd gamma + beta          (unfused fallback)
template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_ln_apply(const float* __restrict__ x,
                                                             const cf* __restrict__ stats,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             float* __restrict__ h, long long rows,
                                                             int D) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  Vec<VEC> gm[CH], bt[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (lane + 64 * c) * VEC;
#pragma unroll
    for (int i = 0; i < VEC; ++i) { gm[c].v[i] = 1.f; bt[c].v[i] = 0.f; }
    if (e < D) {
      if (gamma) gm[c].load_cached(gamma + e);
      if (beta) bt[c].load_cached(beta + e);
    }
  }
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows;
       row += (long long)gridDim.x * ROW_WAVES) {
    const cf st = stats[row];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      if (e < D) {
        Vec<VEC> xv;
        xv.load(x + (size_t)row * D + e);
#pragma unroll
        for (int i = 0; i < VEC; ++i) xv.v[i] = fmaf((xv.v[i] - st.x) * st.y, gm[c].v[i], bt[c].v[i]);
        xv.store(h + (size_t)row * D + e);
      }
    }
  }
}

// y += x      (unfused fallback: the residual)
__global__ void k_add_rows(float* __restrict__ y, const float* __restrict__ x, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x)
    y[i] += x[i];
}

// LayerNorm backward + the residual branch, in place over grad_h:
//   xh = (x - mean) rstd ; u = gamma grad_h ; grad_x = g + rstd (u - mean_d(u) - xh mean_d(u xh))
// and per block:  part[blk][0][d] = sum_rows grad_h xh   (grad_gamma),  part[blk][1][d] = sum_rows grad_h.
template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_ln_bwd(float* __restrict__ gh_dx,
                                                           const float* __restrict__ x,
                                                           const float* __restrict__ g,
                                                           const cf* __restrict__ stats,
                                                           const float* __restrict__ gamma,
                                                           float* __restrict__ part, long long rows,
                                                           int D) {
  __shared__ float red[ROW_WAVES][2][64 * VEC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_d = 1.f / (float)D;
  Vec<VEC> gm[CH], ag[CH], ab[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (lane + 64 * c) * VEC;
#pragma unroll
    for (int i = 0; i < VEC; ++i) { gm[c].v[i] = 1.f; ag[c].v[i] = 0.f; ab[c].v[i] = 0.f; }
    if (e < D && gamma) gm[c].load_cached(gamma + e);
  }
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows;
       row += (long long)gridDim.x * ROW_WAVES) {
    const size_t o = (size_t)row * D;
    Vec<VEC> hv[CH], xv[CH], gv[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      if (e < D) {
        hv[c].load_cached(gh_dx + o + e);      // just written by the transform: may still be in cache
        xv[c].load(x + o + e);
        gv[c].load(g + o + e);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { hv[c].v[i] = 0.f; xv[c].v[i] = 0.f; gv[c].v[i] = 0.f; }
      }
    }
    const cf st = stats[row];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float xh = e < D ? (xv[c].v[i] - st.x) * st.y : 0.f;
        const float gmv = gm[c].v[i];           // read before hv: the operand order of gamma * grad_h
        hv[c].v[i] = ln_bwd_acc(hv[c].v[i], xh, gmv, ag[c].v[i], ab[c].v[i], s1, s2);
        xv[c].v[i] = xh;
      }
    }
    const float m1 = wave_sum(s1) * inv_d, m2 = wave_sum(s2) * inv_d;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      if (e < D) {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
          gv[c].v[i] = fmaf(st.y, hv[c].v[i] - m1 - xv[c].v[i] * m2, gv[c].v[i]);
        gv[c].store(gh_dx + o + e);
      }
    }
  }
  // block partials: waves are added in index order
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
          part[((size_t)blockIdx.x * 2 + 0) * D + e + i] = a0;
          part[((size_t)blockIdx.x * 2 + 1) * D + e + i] = a1;
        }
      }
    }
    __syncthreads();
  }
}

// The same with 2-byte rows: grad_h is read from an f32 scratch of its own, x and g in the element type IO, and grad_x
// is written in IO, rounded once -- not in place.  The arithmetic and its order are k_ln_bwd's, so grad_x is its
// grad_x rounded and the partials are its partials.  A copy, not a shared body: with one, k_ln_bwd<4, .> compiled to
// other machine code (tools/kdiff.py), as with every helper spelling before.
template <int VEC, int CH, int IO>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_ln_bwd_io(const float* __restrict__ gh,
                                                              const io_elem<IO>* __restrict__ x,
                                                              const io_elem<IO>* __restrict__ g,
                                                              io_elem<IO>* __restrict__ dx,
                                                              const cf* __restrict__ stats,
                                                              const float* __restrict__ gamma,
                                                              float* __restrict__ part, long long rows,
                                                              int D) {
  __shared__ float red[ROW_WAVES][2][64 * VEC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_d = 1.f / (float)D;
  Vec<VEC> gm[CH], ag[CH], ab[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (lane + 64 * c) * VEC;
#pragma unroll
    for (int i = 0; i < VEC; ++i) { gm[c].v[i] = 1.f; ag[c].v[i] = 0.f; ab[c].v[i] = 0.f; }
    if (e < D && gamma) gm[c].load_cached(gamma + e);
  }
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows;
       row += (long long)gridDim.x * ROW_WAVES) {
    const size_t o = (size_t)row * D;
    Vec<VEC> hv[CH], xv[CH], gv[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      if (e < D) {
        hv[c].load_cached(gh + o + e);
        load_io<IO>(xv[c], x + o + e);
        load_io<IO>(gv[c], g + o + e);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { hv[c].v[i] = 0.f; xv[c].v[i] = 0.f; gv[c].v[i] = 0.f; }
      }
    }
    const cf st = stats[row];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float xh = e < D ? (xv[c].v[i] - st.x) * st.y : 0.f;
        const float gmv = gm[c].v[i];           // read before hv: the operand order of gamma * grad_h
        hv[c].v[i] = ln_bwd_acc(hv[c].v[i], xh, gmv, ag[c].v[i], ab[c].v[i], s1, s2);
        xv[c].v[i] = xh;
      }
    }
    const float m1 = wave_sum(s1) * inv_d, m2 = wave_sum(s2) * inv_d;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      if (e < D) {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
          gv[c].v[i] = fmaf(st.y, hv[c].v[i] - m1 - xv[c].v[i] * m2, gv[c].v[i]);
        store_io<IO>(gv[c], dx + o + e);
      }
    }
  }
  // block partials: waves are added in index order
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
          part[((size_t)blockIdx.x * 2 + 0) * D + e + i] = a0;
          part[((size_t)blockIdx.x * 2 + 1) * D + e + i] = a1;
        }
      }
    }
    __syncthreads();
  }
}

// out[which][d] = sum_blk part[blk][which][d]; 16 channels x 64 block groups per workgroup, groups
// added in index order (bitwise reproducible).  2 D/16 workgroups: 32 at D = 256.
__global__ __launch_bounds__(1024) void k_ln_colsum(const float* __restrict__ part, int nblk, int D,
                                                    float* __restrict__ g_gamma,
                                                    float* __restrict__ g_beta) {
  __shared__ float red[64][17];
  const int tx = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int d = blockIdx.x * 16 + tx, which = blockIdx.y;
  float acc = 0.f;
  if (d < D) {
    int b = grp;
    for (; b + 64 * 32 <= nblk; b += 64 * 32) {      // all of a thread's loads in one batch
      float v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = part[((size_t)(b + 64 * u) * 2 + which) * D + d];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += v[u];
    }
    for (; b + 64 * 8 <= nblk; b += 64 * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[((size_t)(b + 64 * u) * 2 + which) * D + d];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; b < nblk; b += 64) acc += part[((size_t)b * 2 + which) * D + d];
  }
  red[grp][tx] = acc;
  __syncthreads();
  if (grp == 0 && d < D) {
    float s = 0.f;
#pragma unroll 8
    for (int g2 = 0; g2 < 64; ++g2) s += red[g2][tx];
    float* out = which == 0 ? g_gamma : g_beta;
    if (out) out[d] = s;
  }
}

// out = mask * scale * in over (B, row_elems): the same mask function as the fused epilogues
__global__ void k_dropout_rows(const float* __restrict__ in, float* __restrict__ out, int B,
                               long long row_elems, unsigned thr, float scale,
                               const unsigned long long* __restrict__ rng) {
  const unsigned long long s0 = rng[0], s1 = rng[1];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const unsigned key = drop_row_key(s0, s1, b);
    const size_t base = (size_t)b * (size_t)row_elems;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < row_elems;
         e += (long long)gridDim.x * blockDim.x) {
      const unsigned h = drop_hash((unsigned)((unsigned long long)e >> 1), key);
      const unsigned u = (e & 1) ? (h >> 16) : (h & 0xffffu);
      out[base + e] = u >= thr ? in[base + e] * scale : 0.f;
    }
  }
}

__global__ void k_rng_next(unsigned long long* state, unsigned long long* saved) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const unsigned long long a = state[0], c = state[1];
    saved[0] = a; saved[1] = c;
    state[1] = c + 1;
  }
}

// (VEC, CH) of a D-wide row: Vec<4> tiles up to 16 chunks when D % 4 == 0, else scalar tiles of 1, 4, 16
template <typename Fn>
bool ln_dispatch(int D, Fn f) {
  return D % 4 == 0 ? row_dispatch<4, 16>(D, f) : row_dispatch<1, 16, 4>(D, f);
}

// ---- the O-neuron head, O = 1 or 2 (reference fft_lm/phase_clock.py:53,65, fft_lm/segmentation_head.py:43,55) ---------
// A Linear with one or two output columns over all B T rows is a row reduction bound by the read of h: one wavefront per
// row, the O weight rows held in registers across the wave's row walk, one wave sum per output.
template <int VEC, int CH, int O>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_head_fwd(const float* __restrict__ h, const float* __restrict__ w,
                                                             const float* __restrict__ b, float* __restrict__ y,
                                                             long long rows, int D) {
  constexpr int R = CH <= 2 ? 2 : 1;          // rows in flight per wavefront (as k_ln_stats)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  Vec<VEC> wr[O][CH];
  float bias[O];
#pragma unroll
  for (int o = 0; o < O; ++o) {
    row_load_cached(wr[o], w + (size_t)o * D, D, lane, 0.f);
    bias[o] = b ? b[o] : 0.f;
  }
  const long long step = (long long)gridDim.x * ROW_WAVES;
  for (long long row0 = (long long)blockIdx.x * ROW_WAVES + wv; row0 < rows; row0 += R * step) {
    Vec<VEC> hv[R][CH];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const long long row = row0 + q * step;
      if (row < rows) row_load(hv[q], h + (size_t)row * D, D, lane);
      else zero(hv[q]);
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const long long row = row0 + q * step;
#pragma unroll
      for (int o = 0; o < O; ++o) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int i = 0; i < VEC; ++i) s = fmaf(hv[q][c].v[i], wr[o][c].v[i], s);
        s = wave_sum(s);
        if (lane == 0 && row < rows) y[row * O + o] = s + bias[o];
      }
    }
  }
}

// grad_h[r, :] = sum_o g[r, o] w[o, :] (gh null: skipped), and per block the partials of grad_w[o, e] = sum_r g[r, o]
// h[r, e] in part_w's (2, D) slab (row 1 is zero for O = 1) and of grad_b[o] = sum_r g[r, o] in part_b's pair: what
// k_ln_colsum adds over the blocks in a fixed order.  A null part_w skips the read of h, a null part_b the sums of g.
template <int VEC, int CH, int O>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_head_bwd(const float* __restrict__ g, const float* __restrict__ h,
                                                             const float* __restrict__ w, float* __restrict__ gh,
                                                             float* __restrict__ part_w, float* __restrict__ part_b,
                                                             long long rows, int D) {
  __shared__ float red[ROW_WAVES][2][64 * VEC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  Vec<VEC> wr[O][CH], acc[2][CH];
#pragma unroll
  for (int o = 0; o < O; ++o) row_load_cached(wr[o], gh ? w + (size_t)o * D : nullptr, D, lane, 0.f);
  zero(acc[0]);
  zero(acc[1]);
  float gb[2] = {0.f, 0.f};
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows;
       row += (long long)gridDim.x * ROW_WAVES) {
    float gv[O];
#pragma unroll
    for (int o = 0; o < O; ++o) {
      gv[o] = g[row * O + o];
      gb[o] += gv[o];
    }
    const size_t off = (size_t)row * D;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      if (e < D) {
        if (part_w) {
          Vec<VEC> hv;
          hv.load(h + off + e);
#pragma unroll
          for (int o = 0; o < O; ++o)
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[o][c].v[i] = fmaf(gv[o], hv.v[i], acc[o][c].v[i]);
        }
        if (gh) {
          Vec<VEC> ov;
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            float s = gv[0] * wr[0][c].v[i];
            if constexpr (O == 2) s = fmaf(gv[1], wr[1][c].v[i], s);
            ov.v[i] = s;
          }
          ov.store(gh + off + e);
        }
      }
    }
  }
  if (part_w) block_partials(acc[0], acc[1], part_w + (size_t)blockIdx.x * 2 * D, D, 0, D, red, lane, wv);
  if (part_b) {                               // waves are added in index order
    if (lane == 0) { red[wv][0][0] = gb[0]; red[wv][1][0] = gb[1]; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < ROW_WAVES; ++w2) { a0 += red[w2][0][0]; a1 += red[w2][1][0]; }
      part_b[(size_t)blockIdx.x * 2] = a0;
      part_b[(size_t)blockIdx.x * 2 + 1] = a1;
    }
  }
}

// ---- softmax cross-entropy (reference fft_lm/dual_head.py:176-188) ----------------------------------------------------
// Bound by the read of the logits (forward) and by that read plus the write of the gradient (backward).  A row's
// target is uniform over the wavefront resp. workgroup that owns the row, so the test for an ignored row skips the row's
// loads without divergence.  Exponentials are __expf of an argument <= 0 (relative error about 1e-7 |arg|).
constexpr float XENT_NINF = -__builtin_huge_valf();

// Maximum over the 64 lanes, returned in every lane: wave_sum's DPP steps, a lane without a source keeping its own value
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_keep(float v) {
  const int w = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(w, w, CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_keep<0x111, 0xf>(v));
  v = fmaxf(v, dpp_keep<0x112, 0xf>(v));
  v = fmaxf(v, dpp_keep<0x114, 0xf>(v));
  v = fmaxf(v, dpp_keep<0x118, 0xf>(v));      // lane 15 of each row holds the row maximum
  v = fmaxf(v, dpp_keep<0x142, 0xa>(v));
  v = fmaxf(v, dpp_keep<0x143, 0xc>(v));      // lane 63 holds the maximum
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// The reference point of a (max, sum) pair: the maximum, or 0 while everything seen is -inf, so that no exponent is
// ever formed as -inf - -inf.  exp(m - xent_ref(M)) rescales a sum kept relative to m <= M (0 for m = -inf).
__device__ __forceinline__ float xent_ref(float m) { return m == XENT_NINF ? 0.f : m; }

// One element of the gradient from the row's (m, d) = (max, log sum exp(x - max)): the pair is kept apart because
// m + d rounded to one float loses d beside a large |m|, and exp(x - lse) would then be 1 where it is 1 / n.
__device__ __forceinline__ float xent_grad(float v, float m, float d, float sc, bool hit) {
  return (__expf((v - m) - d) - (hit ? 1.f : 0.f)) * sc;
}

// s_r of the backward; NaN for a target outside [0, V)
__device__ __forceinline__ float xent_scale(const float* g, const float* count, long long row, int reduction, bool in_range) {
  if (!in_range) return __builtin_nanf("");
  return reduction == XENT_NONE ? g[row] : reduction == XENT_MEAN ? g[0] / count[0] : g[0];
}

// One (sum, count) pair per block from the per-wave pairs, waves added in index order.
__device__ __forceinline__ void xent_block_partial(float sum, float cnt, float* part, float (*red)[2], int lane, int wv,
                                                   int waves) {
  if (lane == 0) { red[wv][0] = sum; red[wv][1] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a0 = 0.f, a1 = 0.f;
    for (int w2 = 0; w2 < waves; ++w2) { a0 += red[w2][0]; a1 += red[w2][1]; }
    part[(size_t)blockIdx.x * 2] = a0;
    part[(size_t)blockIdx.x * 2 + 1] = a1;
  }
}

// Register rows: one wavefront per row, the row in Vec<VEC>[CH], the padding at -inf.
template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_xent_fwd(const float* __restrict__ x, long long stride,
                                                             const long long* __restrict__ tg, long long ignore,
                                                             float* __restrict__ loss_rows, float* __restrict__ lse,
                                                             float* __restrict__ part, long long rows, int V) {
  __shared__ float red[ROW_WAVES][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float acc = 0.f, cnt = 0.f;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows; row += (long long)gridDim.x * ROW_WAVES) {
    const long long t = tg[row];
    if (t == ignore) {
      if (lane == 0) {
        lse[2 * row] = lse[2 * row + 1] = 0.f;
        if (loss_rows) loss_rows[row] = 0.f;
      }
      continue;
    }
    const float* p = x + row * stride;
    Vec<VEC> xv[CH];
    float m = XENT_NINF;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      if (e < V) xv[c].load(p + e);
      else
#pragma unroll
        for (int i = 0; i < VEC; ++i) xv[c].v[i] = XENT_NINF;
#pragma unroll
      for (int i = 0; i < VEC; ++i) m = fmaxf(m, xv[c].v[i]);
    }
    m = wave_max(m);
    const float ref = xent_ref(m);
    float s = 0.f, xt = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        s += __expf(xv[c].v[i] - ref);
        if ((long long)(e + i) == t) xt = xv[c].v[i];
      }
    }
    s = wave_sum(s);
    xt = wave_sum(xt);                         // one lane holds the target's logit, the others 0
    const float d = logf(s);
    const float lr = (t >= 0 && t < V) ? d - (xt - m) : __builtin_nanf("");
    acc += lr;
    cnt += 1.f;
    if (lane == 0) {
      lse[2 * row] = m;
      lse[2 * row + 1] = d;
      if (loss_rows) loss_rows[row] = lr;
    }
  }
  xent_block_partial(acc, cnt, part, red, lane, wv, ROW_WAVES);
}

template <int VEC, int CH>
__global__ __launch_bounds__(64 * ROW_WAVES) void k_xent_bwd(const float* __restrict__ g, const float* __restrict__ x,
                                                             long long stride, const long long* __restrict__ tg,
                                                             long long ignore, int reduction,
                                                             const float* __restrict__ lse, const float* __restrict__ count,
                                                             float* __restrict__ grad, long long rows, int V) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wv; row < rows; row += (long long)gridDim.x * ROW_WAVES) {
    const long long t = tg[row];
    const bool live = t != ignore;
    const float* p = x + row * stride;
    float* q = grad + row * (long long)V;
    float m = 0.f, d = 0.f, sc = 0.f;
    if (live) {
      m = lse[2 * row];
      d = lse[2 * row + 1];
      sc = xent_scale(g, count, row, reduction, t >= 0 && t < V);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (lane + 64 * c) * VEC;
      if (e < V) {
        Vec<VEC> v;
        if (live) {
          v.load(p + e);
#pragma unroll
          for (int i = 0; i < VEC; ++i)
            v.v[i] = xent_grad(v.v[i], m, d, sc, (long long)(e + i) == t);
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) v.v[i] = 0.f;
        }
        v.store(q + e);
      }
    }
  }
}

// Streaming rows: one workgroup per row, workgroups walking the rows.  A row starts at any 4-byte address: elements
// [0, head) up to the first 16-byte boundary one per thread, then nvec 16-byte chunks, thread i taking chunks i, i + 256,
// ..., then the last V - head - 4 nvec < 4 elements one per thread.
struct XentSpan {
  int head, nvec, tail0;                      // tail0: index of the first tail element
};
__device__ __forceinline__ XentSpan xent_span(const float* p, int V) {
  XentSpan sp;
  const int to_align = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;
  sp.head = to_align < V ? to_align : V;
  sp.nvec = (V - sp.head) >> 2;
  sp.tail0 = sp.head + 4 * sp.nvec;
  return sp;
}

// (m, s) += one element / one chunk: s stays relative to xent_ref(m)
__device__ __forceinline__ void xent_add(float& m, float& s, float v) {
  const float mn = fmaxf(m, v);
  const float ref = xent_ref(mn);
  s = s * __expf(m - ref) + __expf(v - ref);
  m = mn;
}
__device__ __forceinline__ void xent_add4(float& m, float& s, const f32x4 w) {
  const float mn = fmaxf(fmaxf(m, fmaxf(w.x, w.y)), fmaxf(w.z, w.w));
  const float ref = xent_ref(mn);
  s = s * __expf(m - ref) + ((__expf(w.x - ref) + __expf(w.y - ref)) + (__expf(w.z - ref) + __expf(w.w - ref)));
  m = mn;
}
__device__ __forceinline__ float xent_pick(const f32x4 w, int j, long long t, float xt) {
  const long long d = t - j;
  return d == 0 ? w.x : d == 1 ? w.y : d == 2 ? w.z : d == 3 ? w.w : xt;
}

__global__ __launch_bounds__(XENT_BLOCK) void k_xent_fwd_stream(const float* __restrict__ x, long long stride,
                                                                const long long* __restrict__ tg, long long ignore,
                                                                float* __restrict__ loss_rows, float* __restrict__ lse,
                                                                float* __restrict__ part, long long rows, int V) {
  constexpr int WAVES = XENT_BLOCK / 64;
  __shared__ float red[WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float acc = 0.f, cnt = 0.f;                 // thread 0's are the block's
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const long long t = tg[row];
    if (t == ignore) {
      if (tid == 0) {
        lse[2 * row] = lse[2 * row + 1] = 0.f;
        if (loss_rows) loss_rows[row] = 0.f;
      }
      continue;
    }
    const float* p = x + row * stride;
    const XentSpan sp = xent_span(p, V);
    float m = XENT_NINF, s = 0.f, xt = 0.f;
    if (tid < sp.head) {
      const float v = __builtin_nontemporal_load(p + tid);
      xent_add(m, s, v);
      if (tid == t) xt = v;
    }
    const f32x4* pv = reinterpret_cast<const f32x4*>(p + sp.head);
    int i = tid;
    for (; i + 3 * XENT_BLOCK < sp.nvec; i += 4 * XENT_BLOCK) {      // four chunks in flight
      f32x4 w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u] = __builtin_nontemporal_load(pv + i + u * XENT_BLOCK);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xent_add4(m, s, w[u]);
        xt = xent_pick(w[u], sp.head + 4 * (i + u * XENT_BLOCK), t, xt);
      }
    }
    for (; i < sp.nvec; i += XENT_BLOCK) {
      const f32x4 w = __builtin_nontemporal_load(pv + i);
      xent_add4(m, s, w);
      xt = xent_pick(w, sp.head + 4 * i, t, xt);
    }
    if (tid < V - sp.tail0) {
      const float v = __builtin_nontemporal_load(p + sp.tail0 + tid);
      xent_add(m, s, v);
      if (sp.tail0 + tid == t) xt = v;
    }
    // threads -> wave -> workgroup, each step relative to the wider maximum, waves in index order
    const float mw = wave_max(m);
    const float sw = wave_sum(s * __expf(m - xent_ref(mw)));
    const float xw = wave_sum(xt);
    __syncthreads();                          // the previous row's reads of red are done
    if (lane == 0) { red[wv][0] = mw; red[wv][1] = sw; red[wv][2] = xw; }
    __syncthreads();
    float mb = red[0][0];
#pragma unroll
    for (int w2 = 1; w2 < WAVES; ++w2) mb = fmaxf(mb, red[w2][0]);
    const float ref = xent_ref(mb);
    float sb = 0.f, xb = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < WAVES; ++w2) {
      sb += red[w2][1] * __expf(red[w2][0] - ref);
      xb += red[w2][2];
    }
    const float d = logf(sb);
    const float lr = (t >= 0 && t < V) ? d - (xb - mb) : __builtin_nanf("");
    acc += lr;
    cnt += 1.f;
    if (tid == 0) {
      lse[2 * row] = mb;
      lse[2 * row + 1] = d;
      if (loss_rows) loss_rows[row] = lr;
    }
  }
  if (tid == 0) {
    part[(size_t)blockIdx.x * 2] = acc;
    part[(size_t)blockIdx.x * 2 + 1] = cnt;
  }
}

// The gradient row is dense, so its 16-byte boundaries need not be the logits row's: the span is the gradient row's
// (every store aligned), and the logits are read as 16-byte chunks only where the two rows are co-aligned.
__global__ __launch_bounds__(XENT_BLOCK) void k_xent_bwd_stream(const float* __restrict__ g, const float* __restrict__ x,
                                                                long long stride, const long long* __restrict__ tg,
                                                                long long ignore, int reduction,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ count, float* __restrict__ grad,
                                                                long long rows, int V) {
  const int tid = threadIdx.x;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const long long t = tg[row];
    const bool live = t != ignore;
    const float* p = x + row * stride;
    float* q = grad + row * (long long)V;
    const XentSpan sp = xent_span(q, V);
    const bool co = (((uintptr_t)p ^ (uintptr_t)q) & 15u) == 0;
    float m = 0.f, d = 0.f, sc = 0.f;
    if (live) {
      m = lse[2 * row];
      d = lse[2 * row + 1];
      sc = xent_scale(g, count, row, reduction, t >= 0 && t < V);
    }
    if (tid < sp.head)
      __builtin_nontemporal_store(live ? xent_grad(__builtin_nontemporal_load(p + tid), m, d, sc, tid == t) : 0.f, q + tid);
    f32x4* qv = reinterpret_cast<f32x4*>(q + sp.head);
    for (int i = tid; i < sp.nvec; i += XENT_BLOCK) {
      const int j = sp.head + 4 * i;
      f32x4 w;
      if (!live) {
        w.x = w.y = w.z = w.w = 0.f;
      } else {
        if (co) {
          w = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + j));
        } else {
          w.x = __builtin_nontemporal_load(p + j);
          w.y = __builtin_nontemporal_load(p + j + 1);
          w.z = __builtin_nontemporal_load(p + j + 2);
          w.w = __builtin_nontemporal_load(p + j + 3);
        }
        const long long dt = t - j;
        w.x = xent_grad(w.x, m, d, sc, dt == 0);
        w.y = xent_grad(w.y, m, d, sc, dt == 1);
        w.z = xent_grad(w.z, m, d, sc, dt == 2);
        w.w = xent_grad(w.w, m, d, sc, dt == 3);
      }
      __builtin_nontemporal_store(w, qv + i);
    }
    if (tid < V - sp.tail0) {
      const int j = sp.tail0 + tid;
      __builtin_nontemporal_store(live ? xent_grad(__builtin_nontemporal_load(p + j), m, d, sc, j == t) : 0.f, q + j);
    }
  }
}

// loss[0] = sum of the partial sums (/ the count for the mean), count[0] = sum of the partial counts: thread i adds
// partials [i per, (i + 1) per) in order, the wave sum adds the threads, thread 0 the waves: one fixed order.
__global__ __launch_bounds__(XENT_BLOCK) void k_xent_finish(const float* __restrict__ part, int nblk, int reduction,
                                                            float* __restrict__ loss, float* __restrict__ count) {
  __shared__ float red[XENT_BLOCK / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int per = (nblk + XENT_BLOCK - 1) / XENT_BLOCK;
  float a0 = 0.f, a1 = 0.f;
  for (int b = tid * per; b < nblk && b < (tid + 1) * per; ++b) {
    a0 += part[2 * (size_t)b];
    a1 += part[2 * (size_t)b + 1];
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if (lane == 0) { red[wv][0] = a0; red[wv][1] = a1; }
  __syncthreads();
  if (tid == 0) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < XENT_BLOCK / 64; ++w2) { s0 += red[w2][0]; s1 += red[w2][1]; }
    count[0] = s1;
    if (reduction == XENT_MEAN) loss[0] = s0 / s1;
    else if (reduction == XENT_SUM) loss[0] = s0;
  }
}

}  // namespace

int ln_num_blocks(long long rows) {
  long long b = (rows + ROW_WAVES - 1) / ROW_WAVES;
  return (int)(b < 1 ? 1 : b > LN_MAX_BLOCKS ? LN_MAX_BLOCKS : b);
}

bool ln_supported(int D) { return D >= 1 && (D % 4 == 0 ? D <= LN_MAX_D : D <= LN_MAX_D_ODD); }

hipError_t launch_dropout_rows(const float* in, float* out, int B, long long row_elems, unsigned thr,
                               float scale, const unsigned long long* rng, hipStream_t s) {
  if (B <= 0 || row_elems <= 0) return hipSuccess;
  const long long nb = (row_elems + 255) / 256;
  dim3 grid((unsigned)(nb < 4096 ? nb : 4096), (unsigned)(B < 64 ? B : 64));
  hipLaunchKernelGGL(k_dropout_rows, grid, dim3(256), 0, s, in, out, B, row_elems, thr, scale, rng);
  return hipGetLastError();
}

hipError_t launch_rng_next(unsigned long long* state, unsigned long long* saved, hipStream_t s) {
  hipLaunchKernelGGL(k_rng_next, dim3(1), dim3(64), 0, s, state, saved);
  return hipGetLastError();
}

hipError_t launch_ln_stats(const float* x, cf* stats, long long rows, int D, float eps,
                           hipStream_t s) {
  ln_dispatch(D, [&](auto vec, auto ch) {
    row_launch(k_ln_stats<decltype(vec)::value, decltype(ch)::value>, rows, s, x, stats, rows, D, eps);
  });
  return hipGetLastError();
}

// 2-byte rows: Vec<4> chunks only, 8 bytes per lane.  (D % 4 != 0 stays on the up-cast route: the f32 kernels walk such
// a row one element per lane, and any wider 2-byte chunk would add the row sums in another order.)
bool ln_io_supported(int D) { return D % 4 == 0 && ln_supported(D); }

template <int IO>
static void launch_ln_stats_t(const void* x, cf* stats, long long rows, int D, float eps, hipStream_t s) {
  row_dispatch<4, 16>(D, [&](auto vec, auto ch) {
    row_launch(k_ln_stats<decltype(vec)::value, decltype(ch)::value, IO>, rows, s, (const io_elem<IO>*)x, stats, rows,
               D, eps);
  });
}
hipError_t launch_ln_stats_io(const void* x, cf* stats, long long rows, int D, float eps, hipStream_t s, int io) {
  if (!ln_io_supported(D) || (io != 1 && io != 2)) return hipErrorInvalidValue;
  if (io == 1) launch_ln_stats_t<1>(x, stats, rows, D, eps, s); else launch_ln_stats_t<2>(x, stats, rows, D, eps, s);
  return hipGetLastError();
}

hipError_t launch_ln_apply(const float* x, const cf* stats, const float* gamma, const float* beta,
                           float* h, long long rows, int D, hipStream_t s) {
  ln_dispatch(D, [&](auto vec, auto ch) {
    row_launch(k_ln_apply<decltype(vec)::value, decltype(ch)::value>, rows, s, x, stats, gamma, beta, h,
               rows, D);
  });
  return hipGetLastError();
}

hipError_t launch_add_rows(float* y, const float* x, size_t total, hipStream_t s) {
  if (total == 0) return hipSuccess;
  const size_t nb = (total + 255) / 256;
  hipLaunchKernelGGL(k_add_rows, dim3((unsigned)(nb < 16384 ? nb : 16384)), dim3(256), 0, s, y, x,
                     total);
  return hipGetLastError();
}

hipError_t launch_ln_colsum(const float* part, int nblk, int D, float* g_gamma, float* g_beta, hipStream_t s) {
  if (!g_gamma && !g_beta) return hipSuccess;
  hipLaunchKernelGGL(k_ln_colsum, dim3((D + 15) / 16, 2), dim3(1024), 0, s, part, nblk, D, g_gamma, g_beta);
  return hipGetLastError();
}

hipError_t launch_ln_bwd(float* gh_dx, const float* x, const float* g, const cf* stats,
                         const float* gamma, float* part, float* g_gamma, float* g_beta,
                         long long rows, int D, hipStream_t s) {
  ln_dispatch(D, [&](auto vec, auto ch) {
    row_launch(k_ln_bwd<decltype(vec)::value, decltype(ch)::value>, rows, s, gh_dx, x, g, stats, gamma,
               part, rows, D);
  });
  if (hipError_t e = hipGetLastError()) return e;
  return launch_ln_colsum(part, ln_num_blocks(rows), D, g_gamma, g_beta, s);
}

template <int IO>
static void launch_ln_bwd_t(const float* gh, const void* x, const void* g, void* dx, const cf* stats,
                            const float* gamma, float* part, long long rows, int D, hipStream_t s) {
  row_dispatch<4, 16>(D, [&](auto vec, auto ch) {
    row_launch(k_ln_bwd_io<decltype(vec)::value, decltype(ch)::value, IO>, rows, s, gh, (const io_elem<IO>*)x,
               (const io_elem<IO>*)g, (io_elem<IO>*)dx, stats, gamma, part, rows, D);
  });
}
hipError_t launch_ln_bwd_io(const float* gh, const void* x, const void* g, void* dx, const cf* stats,
                            const float* gamma, float* part, float* g_gamma, float* g_beta, long long rows, int D,
                            hipStream_t s, int io) {
  if (!ln_io_supported(D) || (io != 1 && io != 2)) return hipErrorInvalidValue;
  if (io == 1) launch_ln_bwd_t<1>(gh, x, g, dx, stats, gamma, part, rows, D, s);
  else launch_ln_bwd_t<2>(gh, x, g, dx, stats, gamma, part, rows, D, s);
  if (hipError_t e = hipGetLastError()) return e;
  return launch_ln_colsum(part, ln_num_blocks(rows), D, g_gamma, g_beta, s);
}

size_t head_part_w_bytes(long long R, int C) { return (size_t)ln_num_blocks(R) * 2 * C * sizeof(float); }
size_t head_part_b_bytes(long long R) { return (size_t)ln_num_blocks(R) * 2 * sizeof(float); }

hipError_t launch_head_fwd(const float* h, const float* w, const float* b, float* y, long long R, int C, int O,
                           hipStream_t s) {
  if (!ln_supported(C) || (O != 1 && O != 2)) return hipErrorInvalidValue;
  ln_dispatch(C, [&](auto vec, auto ch) {
    constexpr int V = decltype(vec)::value, H = decltype(ch)::value;
    if (O == 1) row_launch(k_head_fwd<V, H, 1>, R, s, h, w, b, y, R, C);
    else row_launch(k_head_fwd<V, H, 2>, R, s, h, w, b, y, R, C);
  });
  return hipGetLastError();
}

hipError_t launch_head_bwd(const float* g, const float* h, const float* w, float* grad_h, float* grad_w, float* grad_b,
                           float* part_w, float* part_b, long long R, int C, int O, hipStream_t s) {
  if (!ln_supported(C) || (O != 1 && O != 2)) return hipErrorInvalidValue;
  if (!grad_h && !grad_w && !grad_b) return hipSuccess;
  float* pw = grad_w ? part_w : nullptr;
  float* pb = grad_b ? part_b : nullptr;
  ln_dispatch(C, [&](auto vec, auto ch) {
    constexpr int V = decltype(vec)::value, H = decltype(ch)::value;
    if (O == 1) row_launch(k_head_bwd<V, H, 1>, R, s, g, h, w, grad_h, pw, pb, R, C);
    else row_launch(k_head_bwd<V, H, 2>, R, s, g, h, w, grad_h, pw, pb, R, C);
  });
  if (hipError_t e = hipGetLastError()) return e;
  const int nblk = ln_num_blocks(R);
  if (hipError_t e = launch_ln_colsum(pw, nblk, C, grad_w, grad_w && O == 2 ? grad_w + C : nullptr, s)) return e;
  return launch_ln_colsum(pb, nblk, 1, grad_b, grad_b && O == 2 ? grad_b + 1 : nullptr, s);
}

// ---- softmax cross-entropy ---------------------------------------------------------------------------------------------
int xent_num_blocks(long long R) { return (int)(R < 1 ? 1 : R > LN_MAX_BLOCKS ? LN_MAX_BLOCKS : R); }

namespace {

// The kernel family of a call: f(VEC, CH) for register rows -- Vec<4> chunks only where every row of logits and grad
// (null in the forward) starts on a 16-byte boundary, else the one-element-per-lane instances while they reach V --
// and false for the streaming rows.
template <typename Fn>
bool xent_dispatch(int V, const float* logits, long long row_stride, const float* grad, Fn f) {
  const bool rows16 = (((uintptr_t)logits | (uintptr_t)grad) & 15) == 0 && row_stride % 4 == 0;
  if (V % 4 == 0 && V <= LN_MAX_D && rows16) return row_dispatch<4, 16>(V, f);
  if (V <= LN_MAX_D_ODD) return row_dispatch<1, 16, 4>(V, f);
  return false;
}

}  // namespace

hipError_t launch_xent_fwd(const float* logits, long long row_stride, const long long* targets, long long ignore_index,
                           int reduction, float* loss, float* lse, float* count, float* part, long long R, int V,
                           hipStream_t s) {
  float* loss_rows = reduction == XENT_NONE ? loss : nullptr;
  int nblk = ln_num_blocks(R);
  const bool reg = xent_dispatch(V, logits, row_stride, nullptr, [&](auto vec, auto ch) {
    row_launch(k_xent_fwd<decltype(vec)::value, decltype(ch)::value>, R, s, logits, row_stride, targets, ignore_index,
               loss_rows, lse, part, R, V);
  });
  if (!reg) {
    nblk = xent_num_blocks(R);
    hipLaunchKernelGGL(k_xent_fwd_stream, dim3(nblk), dim3(XENT_BLOCK), 0, s, logits, row_stride, targets, ignore_index,
                       loss_rows, lse, part, R, V);
  }
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(k_xent_finish, dim3(1), dim3(XENT_BLOCK), 0, s, (const float*)part, nblk, reduction, loss, count);
  return hipGetLastError();
}

hipError_t launch_xent_bwd(const float* g, const float* logits, long long row_stride, const long long* targets,
                           long long ignore_index, int reduction, const float* lse, const float* count, float* grad,
                           long long R, int V, hipStream_t s) {
  const bool reg = xent_dispatch(V, logits, row_stride, grad, [&](auto vec, auto ch) {
    row_launch(k_xent_bwd<decltype(vec)::value, decltype(ch)::value>, R, s, g, logits, row_stride, targets, ignore_index,
               reduction, lse, count, grad, R, V);
  });
  if (!reg)
    hipLaunchKernelGGL(k_xent_bwd_stream, dim3(xent_num_blocks(R)), dim3(XENT_BLOCK), 0, s, g, logits, row_stride, targets,
                       ignore_index, reduction, lse, count, grad, R, V);
  return hipGetLastError();
}

}  // namespace smx
