// smx_api.hip -- C ABI (include/smx.h): validation, plan selection, twiddle-table cache, dispatch.
#include <initializer_list>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "../../include/smx.h"
#include "smx_kernels.h"
#include "smx_tables.h"

using namespace smx;

namespace {

thread_local std::string t_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  t_err = buf;
  return code;
}

// (the sticky error of somebody else's earlier failure -- e.g. an invalidated stream capture -- is
// cleared first, so that it is not reported as the failure of this launch)
#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    (void)hipGetLastError();                                                             \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(SMX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                  __FILE__, __LINE__);                                                   \
  } while (0)

// Plan knobs.  Process-wide defaults (smx_set_option) and, on top of them, a per-thread stack of overrides
// (smx_options_push / smx_options_pop): plan choice is an argument of the calling context, two users of one
// process can run different plans, and nothing a caller memoises per shape goes stale behind its back --
// g_opt_epoch changes with every change of a default.
std::atomic<int> o_nsplit{0}, o_placement{2}, o_force_direct{0}, o_round{512}, o_full8{1}, o_fourstep{1};
std::atomic<int> o_fs_bgroups{0}, o_fold_gradw{0}, o_decim16{1}, o_conv1{1}, o_st_plain{-1};
// placement of the write-back rows (store_layout, smx_kernels.h), forward and backward launches apart.  Not a member of
// smx_options (the struct has no size field to grow by): process-wide only.  The store policy never changes a result or
// a workspace layout, so the two halves of a call pair need not agree on it.
// -2 (default) = by the rule in decim_args.
std::atomic<int> o_st_layout_fwd{-2}, o_st_layout_bwd{-2};
std::atomic<unsigned long long> g_opt_epoch{1}, g_tab_epoch{1};
constexpr int OPT_DEPTH = 8;
thread_local smx_options t_opt_stack[OPT_DEPTH];
thread_local int t_opt_depth = 0;

smx_options default_opts() {
  smx_options o;
  o.nsplit = o_nsplit.load(); o.placement = o_placement.load(); o.round = o_round.load();
  o.force_direct = o_force_direct.load(); o.full8 = o_full8.load(); o.fourstep = o_fourstep.load();
  o.fs_bgroups = o_fs_bgroups.load();
  o.fold_gradw = o_fold_gradw.load();
  o.decim16 = o_decim16.load();
  o.conv1 = o_conv1.load();
  o.st_plain = o_st_plain.load();
  return o;
}
smx_options cur_opts() { return t_opt_depth > 0 ? t_opt_stack[t_opt_depth - 1] : default_opts(); }

// ---- twiddle cache, keyed by (device, N) ---------------------------------------------------------
// Tables are uploaded with a blocking hipMemcpy the first time an N is seen on a device.  That must
// not happen while `stream` is being captured into a hipGraph (the copy would invalidate the capture):
// such a call fails cleanly and asks for smx_prepare(N) up front.  The cache is bounded: past
// `table_cache_entries` distinct (device, N) the least recently used tables are freed after a device
// synchronise (variable-length workloads); hipGraphs captured with an evicted N must be re-captured,
// so keep the bound above the number of sequence lengths a graph-replaying process uses.
struct Tables { cf* tw = nullptr; cf* bt = nullptr; cf* tq = nullptr; cf* v16 = nullptr; cf* b16 = nullptr; };
struct TableEntry { Tables t; std::map<int, cf*> group_bt; unsigned long long used = 0; int pins = 0; };
std::mutex g_mu;
std::map<std::pair<int, int>, TableEntry> g_tables;
unsigned long long g_tick = 0;
std::atomic<int> o_table_cap{256};

// What get_tables hands to a call: the entry stays PINNED until the call has enqueued its launches (the
// destructor runs when the entry point returns), so another thread's eviction cannot free tables between
// the lookup and the launch; once unpinned, the evictor's hipDeviceSynchronize covers the enqueued work.
struct TableRef : Tables {
  std::pair<int, int> key{-1, -1};
  TableRef() = default;
  TableRef(const TableRef&) = delete;
  TableRef& operator=(const TableRef&) = delete;
  ~TableRef() {
    if (key.first < 0) return;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_tables.find(key);
    if (it != g_tables.end() && it->second.pins > 0) --it->second.pins;
  }
};

bool capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  const hipError_t e = hipStreamIsCapturing(s, &st);
  if (e != hipSuccess) { (void)hipGetLastError(); return true; }   // e.g. legacy stream during a global capture
  return st != hipStreamCaptureStatusNone;
}

// Victims: least recently used, on the CURRENT device only (hipDeviceSynchronize below covers exactly that
// device's queues; entries of other devices wait for a call made there), never pinned, never the entry just made.
void evict_locked(int dev, int keepN) {
  while ((int)g_tables.size() > o_table_cap.load()) {
    auto victim = g_tables.end();
    for (auto it = g_tables.begin(); it != g_tables.end(); ++it)
      if (it->first.first == dev && it->first.second != keepN && it->second.pins == 0 &&
          (victim == g_tables.end() || it->second.used < victim->second.used))
        victim = it;
    if (victim == g_tables.end()) return;
    (void)hipDeviceSynchronize();
    (void)hipFree(victim->second.t.tw);
    if (victim->second.t.bt) (void)hipFree(victim->second.t.bt);
    if (victim->second.t.tq) (void)hipFree(victim->second.t.tq);
    if (victim->second.t.v16) (void)hipFree(victim->second.t.v16);
    if (victim->second.t.b16) (void)hipFree(victim->second.t.b16);
    for (auto& kv : victim->second.group_bt) (void)hipFree(kv.second);
    g_tables.erase(victim);
    g_tab_epoch++;
  }
}

int get_tables(int N, TableRef* out, hipStream_t s) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_tables.find({dev, N});
  if (it == g_tables.end()) {
    if (capturing(s))
      return fail(SMX_ERR_UNSUPPORTED,
                  "twiddle tables for N=%d are not on device %d yet and the stream is being captured: "
                  "call smx_prepare(%d) (or run one eager call of this shape) before the capture", N, dev, N);
    TableEntry e;
    std::vector<cf> tw = make_tw(N);
    HIP_TRY(hipMalloc((void**)&e.t.tw, tw.size() * sizeof(cf)));
    HIP_TRY(hipMemcpy(e.t.tw, tw.data(), tw.size() * sizeof(cf), hipMemcpyHostToDevice));
    if (N % M == 0) {
      std::vector<cf> bt = make_bt(N, N / M);
      HIP_TRY(hipMalloc((void**)&e.t.bt, bt.size() * sizeof(cf)));
      HIP_TRY(hipMemcpy(e.t.bt, bt.data(), bt.size() * sizeof(cf), hipMemcpyHostToDevice));
      std::vector<cf> tq = make_tq(N);
      HIP_TRY(hipMalloc((void**)&e.t.tq, tq.size() * sizeof(cf)));
      HIP_TRY(hipMemcpy(e.t.tq, tq.data(), tq.size() * sizeof(cf), hipMemcpyHostToDevice));
    }
    if (N % 16 == 0 && N % M != 0) {           // sixteen-row decimation (make_plan)
      std::vector<cf> v = make_v16(N), bb = make_b16(N);
      HIP_TRY(hipMalloc((void**)&e.t.v16, v.size() * sizeof(cf)));
      HIP_TRY(hipMemcpy(e.t.v16, v.data(), v.size() * sizeof(cf), hipMemcpyHostToDevice));
      HIP_TRY(hipMalloc((void**)&e.t.b16, bb.size() * sizeof(cf)));
      HIP_TRY(hipMemcpy(e.t.b16, bb.data(), bb.size() * sizeof(cf), hipMemcpyHostToDevice));
    }
    g_tables[{dev, N}] = e;
    evict_locked(dev, N);
    it = g_tables.find({dev, N});
  }
  it->second.used = ++g_tick;
  ++it->second.pins;
  out->tw = it->second.t.tw; out->bt = it->second.t.bt; out->tq = it->second.t.tq;
  out->v16 = it->second.t.v16; out->b16 = it->second.t.b16;
  out->key = {dev, N};
  return SMX_OK;
}

// residue twiddles of band group `group` (>= 1; group 0 is Tables::bt); get_tables(N) came first
int get_group_bt(int N, int group, cf** out, hipStream_t s) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_tables.find({dev, N});
  if (it == g_tables.end()) return fail(SMX_ERR_INVALID, "internal: tables of N=%d missing", N);
  auto gt = it->second.group_bt.find(group);
  if (gt != it->second.group_bt.end()) { *out = gt->second; return SMX_OK; }
  if (capturing(s))
    return fail(SMX_ERR_UNSUPPORTED,
                "band-group tables for N=%d are not on the device yet and the stream is being captured: "
                "run one eager call of this shape before the capture", N);
  std::vector<cf> bt = make_bt(N, N / M, group);
  cf* p = nullptr;
  HIP_TRY(hipMalloc((void**)&p, bt.size() * sizeof(cf)));
  HIP_TRY(hipMemcpy(p, bt.data(), bt.size() * sizeof(cf), hipMemcpyHostToDevice));
  it->second.group_bt[group] = p;
  *out = p;
  return SMX_OK;
}

// ---- plan ----------------------------------------------------------------------------------------
// What a shape runs on, resolved once by make_plan (tile_plan for smx_cfft_ex / smx_conv_*):
enum class Kind {
  Direct,     // DFT products
  Sixteen,    // sixteen-row decimation (k_fused16), single launch or tile chunks (nsplit > 1)
  Single,     // up to 512 bins, one fused launch per direction
  Split,      // ... its residue-split form (nsplit > 1): three launches through the workspace
  FourStep,   // k_fs_a / k_fs_f / k_fs_b: more than 512 bins at the tile counts of fs_tiles_filter(); takes precedence
              // over the eight bands and the band groups (option "fourstep" = 0: off)
  Full8,      // N = 2048 with k > 512: the eight-band kernel (k_full8) takes every call that runs forward half and
              // inverse half together; the band groups remain the plan of the phase-split backward (and define the
              // workspace layout, which must not depend on which of the two a call uses)
  Groups,     // more than 512 bins elsewhere: one four-band launch per group of 512 bins + the edge kernels
};
struct Plan {
  Kind kind;
  int path, k, L, nb, nsplit, lc, nwg;
  int groups;     // band groups of 512 bins (1 unless k > 512)
  int nedge;      // bins 512, 1024, ... < k: left to the edge kernels when groups > 1
  int fs_nsplit, fs_lc;   // four-step: tile chunks per (batch row, d-tile), tiles per chunk
  bool pair8;     // N = 2048 with k > 512 and option "full8": smx_rfft_ex / smx_irfft_ex run their eight-band launches
  bool conv1 = false;   // smx_conv_*: one launch per direction (k_conv1: n_fft <= 2048)
  int conv1_nj = 16;    // ... channel pairs per workgroup of that launch (16: 512 threads; 8: 256 threads)
  bool fs() const { return kind == Kind::FourStep; }
  bool full8() const { return kind == Kind::Full8; }
  bool io_native() const { return kind == Kind::Single || kind == Kind::Split; }       // kernels with 2-byte row I/O
  bool block_fused() const { return kind == Kind::Single; }                            // k_fused_blk
  // (row scale: not the eight-band kernel -- it only serves calls that run both halves of the backward together, and a
  // caller must be able to rely on smx_row_scale_supported for every phase split).  The same kinds synthesise from a
  // given spectrum (smx_irfft_ex).
  bool row_scale() const { return io_native() || fs(); }
  bool wide() const { return fs() || full8() || kind == Kind::Groups; }     // more than 512 bins: no fused dropout mask
  bool groups_only() const { return kind == Kind::Groups; }                 // no call of this shape leaves the band groups
};

int check_shape(int B, int N, int D, int F) {
  if (B <= 0 || N <= 0 || D <= 0 || F <= 0)
    return fail(SMX_ERR_INVALID, "shape must be positive: B=%d N=%d D=%d F=%d", B, N, D, F);
  if ((long long)N * D >= (1ll << 40)) return fail(SMX_ERR_INVALID, "N*D too large");
  return SMX_OK;
}

// General problem: x / y have R rows, the transform length is N >= R (rows >= R are zero padding /
// cropped), k bins are kept, k <= min(F, N/2 + 1) -- k = N/2 + 1 includes the Nyquist bin.
// The reference layer's own shapes are R = N, k = min(F, N/2) (layer_shape).
struct Shape { int B, R, D, F, N, k; };
Shape layer_shape(int B, int N, int D, int F) { return Shape{B, N, D, F, N, F < N / 2 ? F : N / 2}; }

int check_shape(const Shape& h) {
  if (int rc = check_shape(h.B, h.N, h.D, h.F)) return rc;
  if (h.R <= 0 || h.R > h.N)
    return fail(SMX_ERR_INVALID, "rows must be in [1, n_fft]: rows=%d n_fft=%d", h.R, h.N);
  if (h.k < 0 || h.k > h.F || h.k > h.N / 2 + 1)
    return fail(SMX_ERR_INVALID, "k must be in [0, min(F, n_fft/2 + 1)]: k=%d F=%d n_fft=%d", h.k, h.F, h.N);
  return SMX_OK;
}
int shape_from(const smx_shape* sh, Shape* out) {
  if (!sh) return fail(SMX_ERR_INVALID, "shape is NULL");
  *out = Shape{sh->B, sh->rows, sh->D, sh->F, sh->n_fft, sh->k};
  return check_shape(*out);
}

// (the tile counts the four-step path takes: fs_tiles_filter / fs_tiles_cfft, smx_kernels.h)

// residue (256-point plan) or tile (sixteen-row plan) chunks per (batch row, d-tile): L = items to cut
static int choose_nsplit(int forced, int nwg, int L, double bytes) {
  int ns = forced;
  if (ns <= 0) {
    // One fused launch per direction whenever the (b, d-tile) pairs alone fill the chip (2 WG/CU).
    // Otherwise the residues are cut into chunks (three more launches, ~30 us of fixed cost):
    //  * large tensors are bandwidth-bound: aim at ONE resident round of 512 workgroups (2 per CU) --
    //    with the XCD-aware placement C3 measured 59 % of the roofline at 8 chunks (512 workgroups)
    //    against 54 % at 16 and 48-51 % at 6, 10, 12 (partial second round);
    //  * small tensors are latency-bound (a workgroup walks 2L tiles at ~2.5 us each): split only if
    //    that walk is longer than the chunked walk plus the fixed cost, and keep one resident round.
    //    (measured: (32,2048,256) 46 us fused vs 65 us split; (2,4096,256) 66 vs 30.)
    ns = 1;
    if (nwg < 384) {
      if (bytes >= 128.0 * (1 << 20)) {
        ns = 512 / nwg;
        if (ns < 1) ns = 1;
      } else {
        int cand = 512 / nwg;
        if (cand > L) cand = L;
        if (cand > 1) {
          const int lc = (L + cand - 1) / cand;
          if (5 * L > 6 * lc + 30) ns = cand;
        }
      }
    }
  }
  return ns;
}

// The four-step tile walk of a decimated plan: one resident round of tile workgroups, as on the split plan.  The
// residue split is off (the band kernels of a phase-split call on this shape run one launch per group).
void tile_plan(Plan& p) {
  p.kind = Kind::FourStep;
  int ns = 512 / p.nwg;
  if (ns < 1) ns = 1;
  if (ns > p.L) ns = p.L;
  p.fs_lc = (p.L + ns - 1) / ns;
  p.fs_nsplit = (p.L + p.fs_lc - 1) / p.fs_lc;
  p.nsplit = 1; p.lc = p.L;
}
// ... as the whole plan of the entries that keep every bin of the packed spectrum (smx_cfft_ex, smx_conv_*), which
// check the tile count themselves
Plan tile_plan(const Shape& h) {
  Plan p{};
  p.path = SMX_PATH_DECIMATED; p.L = h.N / M; p.k = h.N / 2 + 1; p.nb = 4; p.groups = 1;
  p.nwg = h.B * ((h.D + DT - 1) / DT);
  tile_plan(p);
  return p;
}

Plan make_plan(const Shape& h) {
  const int B = h.B, N = h.N, D = h.D;
  Plan p{};
  const smx_options opt = cur_opts();
  p.k = h.k;
  p.groups = 1;
  // (a batch row of 2 GiB or more does not fit the 32-bit offsets of the streaming kernels' buffer accesses, RowBuf)
  const bool rows32 = (unsigned long long)h.R * (unsigned long long)D * 4ull < (1ull << 31);
  const bool fast = !opt.force_direct && N % M == 0 && D % 2 == 0 && p.k >= 1 && rows32;
  if (!fast) {
    // N = 16 P, not a multiple of 256: sixteen-row decimation (k_fused16) for the layer-sized filters (k <= 256;
    // zero-padded rows included: functional.spectral_mix runs N = 8 (odd) as the even bins of 2 N); everything else -- and every call this plan's kernels do not serve (dropout,
    // phase-split backward, synthesis alone) -- runs the DFT products of the direct plan on the same workspace
    if (!opt.force_direct && opt.decim16 != 0 && N % 16 == 0 && N % M != 0 && D % 2 == 0 && p.k >= 1 && p.k <= 256 &&
        p.k <= N / 2) {        // (not the Nyquist bin: its two slots +-N/2 would not cancel to an exact +0 imaginary part)
      p.path = SMX_PATH_DECIM16; p.kind = Kind::Sixteen;
      p.L = (N / 16 + 15) / 16;               // tiles of 16 residues
      p.nb = p.k > 128 ? 2 : 1;
      p.nwg = B * ((D + DT - 1) / DT);
      int ns = choose_nsplit(opt.nsplit, p.nwg, p.L, 4.0 * B * (double)h.R * D);
      if (ns > p.L) ns = p.L;
      p.lc = (p.L + ns - 1) / ns;
      p.nsplit = (p.L + p.lc - 1) / p.lc;
      return p;
    }
    p.path = SMX_PATH_DIRECT; p.kind = Kind::Direct; p.nsplit = 1; return p;
  }
  p.path = SMX_PATH_DECIMATED;
  p.L = N / M;
  // bands by the bins below the Nyquist bin: with k = N/2 + 1 that bin (f = 128 L) is the self-paired
  // edge slot of the NB = L kernels (L in 1, 2, 4), an ordinary +-pair of a wider band set (L = 3), or
  // an edge / interior bin of the band groups
  const int kb = p.k > N / 2 ? N / 2 : p.k;
  p.nb = kb > 256 ? 4 : kb > 128 ? 2 : 1;
  p.nwg = B * ((D + DT - 1) / DT);
  if (kb > 512) {
    p.pair8 = p.L == 8 && opt.full8 != 0;
    p.kind = p.pair8 ? Kind::Full8 : Kind::Groups;
    p.nsplit = 1; p.lc = p.L;
    if (opt.fourstep != 0 && fs_tiles_filter(p.L)) tile_plan(p);
    // More than 512 bins: the four-band kernels run once per group of 512 bins (group g: |f| in
    // [512 g, 512 g + 512), its own residue-twiddle table, later groups add to y); the bins that are
    // multiples of 512 pair across groups and go through the literal-DFT kernels instead.  x is read
    // and y re-written once per group -- 12 B/sample more per extra group, against O(N k) per column
    // for the direct path.  One fused launch per group (no residue split).
    p.groups = (kb + 511) / 512;
    p.nedge = (p.k - 1) / 512;
    return p;
  }
  int ns = choose_nsplit(opt.nsplit, p.nwg, p.L, 4.0 * B * (double)h.R * D);
  if (ns > p.L) ns = p.L;
  p.lc = (p.L + ns - 1) / ns;
  p.nsplit = (p.L + p.lc - 1) / p.lc;
  p.kind = p.nsplit == 1 ? Kind::Single : Kind::Split;
  return p;
}

struct Ws {
  size_t z = 0, zs = 0, s = 0, slab = 0, gbp = 0, spec0 = 0, spec1 = 0, spec2 = 0, lnp = 0, total = 0;
  size_t s_group = 0;            // bytes of one band group's parked spectrum
  size_t edge0 = 0, edge1 = 0;   // (B, nedge, D) complex: edge-bin spectrum / filtered edge bins
  size_t edgep = 0;              // per-chunk partial sums of launch_edge_spectrum
  size_t wt = 0;                 // (k, D) complex: the filter packed for the unpack phase
  size_t fs = 0;                 // four-step path: [B*ndt][L][16][256] complex tile spectra
  size_t gscp = 0;               // four-step path: partial sums of the row-scale gradient
  size_t rows = 0;               // band-group plan: a (B, N, D) float copy of the input (masked g; LayerNorm(x) of the block)
};

// The first WS_HEADER_BYTES of EVERY workspace layout are a reserved header that nothing reads or writes (once the
// flag words of the retired option fold_gradw): every offset below it is pinned, so it stays until it is dropped on purpose.
constexpr size_t WS_HEADER_BYTES = 65536;

Ws ws_layout(const Plan& p, int B, int N, int D) {
  Ws w;
  size_t o = WS_HEADER_BYTES;
  if (p.path == SMX_PATH_DECIM16) {
    w.slab = o; o += al((size_t)B * p.k * D * sizeof(cf));
    w.gbp = o; o += al((size_t)B * D * sizeof(float));
    w.wt = o; o += al((size_t)p.k * D * sizeof(cf));
    const size_t per = (size_t)16 * p.nb * TPB * sizeof(cf);
    w.s = o; o += al((size_t)p.nwg * per);           // filtered spectrum (split plan; parked by a phase-split backward)
    if (p.nsplit > 1) {
      w.z = o; o += al((size_t)p.nwg * p.nsplit * per);
      w.zs = o; o += al((size_t)p.nwg * per);
    }
  }
  if (p.path == SMX_PATH_DECIMATED) {
    const size_t per = (size_t)16 * p.nb * TPB * sizeof(cf);
    w.z = o; o += al((size_t)p.nwg * p.nsplit * per);
    w.zs = o; o += al((size_t)p.nwg * per);
    w.s_group = al((size_t)p.nwg * per);
    w.s = o; o += w.s_group * p.groups;
    if (p.groups > 1) {
      const size_t e = al((size_t)B * p.nedge * D * sizeof(cf));
      w.edge0 = o; o += e;
      w.edge1 = o; o += e;
      w.edgep = o;
      o += al((size_t)edge_chunks(B, N, D) * B * p.nedge * D * 2 * sizeof(double));
      if (p.groups_only()) {     // the group launches re-read their input while the output accumulates: no in-place form
        w.rows = o; o += al((size_t)B * N * D * sizeof(float));
      }
    }
    w.wt = o; o += al((size_t)p.k * D * sizeof(cf));
    if (p.fs()) {
      w.fs = o; o += al((size_t)p.nwg * p.L * EX * sizeof(cf));
      w.gscp = o; o += al((size_t)p.nwg * fs_column_blocks(p.L) * 16 * sizeof(cf));
    }
    w.slab = o; o += al((size_t)B * p.k * D * sizeof(cf));
    w.gbp = o; o += al((size_t)B * D * sizeof(float));
  } else {
    const size_t spec = al((size_t)B * (p.k > 0 ? p.k : 1) * D * sizeof(cf));
    w.spec0 = o; o += spec;
    w.spec1 = o; o += spec;
    w.spec2 = o; o += spec;
  }
  if (ln_supported(D)) {       // grad_gamma / grad_beta partials of smx_block_backward
    w.lnp = o; o += al((size_t)ln_num_blocks((long long)B * N) * 2 * D * sizeof(float));
  }
  w.total = o;
  return w;
}

// THE workspace test: `need` bytes at a 256-byte aligned address
bool ws_usable(const void* ws, size_t bytes, size_t need) { return ws && bytes >= need && !((uintptr_t)ws & 255); }
// ... and its refusal, in one message.  query: the entry that tells the size ("" = none is named)
int need_ws(const void* ws, size_t bytes, size_t need, const char* query) {
  if (ws_usable(ws, bytes, need)) return SMX_OK;
  return fail(SMX_ERR_WORKSPACE, "workspace must be 256-byte aligned and hold %zu bytes%s%s%s", need, *query ? " (" : "",
              query, *query ? ")" : "");
}
// ... or in three: those of the transform entries as they stand; `who` (the entry, "smx_x") goes in front of each and
// `query` (its size query) behind the two that state a size.  misaligned: the code of that fault (include/smx.h: the
// entries differ)
int need_ws(const void* ws, size_t bytes, size_t need, int misaligned, const char* who, const char* query) {
  if (ws_usable(ws, bytes, need)) return SMX_OK;
  const std::string pre = who ? std::string(who) + ": " : "", suf = query ? " (" + std::string(query) + ")" : "";
  if (!ws) return fail(SMX_ERR_WORKSPACE, "%sworkspace is NULL, %zu bytes required%s", pre.c_str(), need, suf.c_str());
  if (bytes < need)
    return fail(SMX_ERR_WORKSPACE, "%sworkspace has %zu bytes, %zu required%s", pre.c_str(), bytes, need, suf.c_str());
  return fail(misaligned, "%sworkspace must be 256-byte aligned", pre.c_str());
}
int need_ws(const Ws& w, const void* ws, size_t bytes) {
  return need_ws(ws, bytes, w.total, SMX_ERR_INVALID, nullptr, nullptr);
}

// THE token source of the entries that read byte tokens (B, T) in place, rows row_stride elements apart: token_bytes 1 /
// 8 -> kind 1 / 2 (uint8 / int64: EmaSrc, launch_word_targets, ...); required: the rows are read (non-NULL, row_stride >= T)
int token_src(const void* tokens, int token_bytes, long long row_stride, long long T, bool required, int* kind) {
  if (token_bytes != 1 && token_bytes != 8) return fail(SMX_ERR_INVALID, "token_bytes must be 1 (uint8) or 8 (int64)");
  if (required && !tokens) return fail(SMX_ERR_INVALID, "tokens must be non-NULL");
  if (required && row_stride < T) return fail(SMX_ERR_INVALID, "row_stride must be at least T");
  if (token_bytes == 8 && ((uintptr_t)tokens & 7)) return fail(SMX_ERR_INVALID, "int64 tokens must be 8-byte aligned");
  *kind = token_bytes == 1 ? 1 : 2;
  return SMX_OK;
}

// elem: bytes per element of the streamed x / y (4; 2 for the 2-byte activations of the _io entries)
// dir: 0 = a forward entry point, 1 = a backward one (which "st_layout_*" option places the write-back rows)
DecimArgs decim_args(const Plan& p, const Tables& t, const Shape& h, char* ws, const Ws& w, int elem = 4, int dir = 0) {
  const int B = h.B, N = h.N, D = h.D, F = h.F;
  DecimArgs a{};
  a.tw = t.tw; a.bt = t.bt; a.tq = t.tq;
  a.g.B = B; a.g.N = N; a.g.D = D; a.g.F = F; a.g.k = p.k; a.g.L = p.L; a.g.R = h.R;
  a.g.inv_n = (float)(1.0 / (double)N);
  if (p.path == SMX_PATH_DECIM16) { a.g.P = N / 16; a.v16 = t.v16; a.b16 = t.b16; }
  const smx_options opt = cur_opts();
  a.placement = opt.placement;
  a.round = opt.round;
  // Store policy of the streamed output (y / grad_x, B R D floats): rows written with the default write-back policy.
  // Measured at step level on five shapes (profiles/r04_store_policy.txt): L2 + Infinity Cache take about 64 MiB of
  // dirty lines per launch sequence at no cost -- those stores retire at cache speed and drain while the next
  // launch reads -- all-streaming stores leave that unused (C2 +9 % step time), all-cached ones overflow it (+13 %).
  // (stated in bytes of the output: a 2-byte output of the same shape is half as many MiB)
  {
    const double mib = (double)elem * B * (double)h.R * D / (1 << 20);
    // (the residue-split plan writes the whole tensor in ONE write-only launch: four rows up to 768 MiB -- C3 0.448 ms
    //  against 0.452 with two and 0.480 with none)
    const int aut = mib <= (p.nsplit > 1 ? 768 : 320) ? 4 : mib <= 768 ? 2 : mib <= 1536 ? 1 : 0;
    a.st_plain = opt.st_plain < 0 ? aut : (opt.st_plain >= 4 ? 4 : opt.st_plain == 3 ? 2 : opt.st_plain);
    a.g.st_plain = a.st_plain;            // (the pointer-addressed tile stores read it from the geometry)
    // WHICH rows (buffer-addressed stores only: store_rows; layouts in smx_kernels.h store_layout).  Rule: the single-launch
    // plan up to 320 MiB of output (C2) spreads them as single rows rotated by tile residue AND wave (layout 4);
    // everything else keeps the thread's first rows (-1).  Why (profiles/store_layout_census.txt;
    // C2 ms per step, 8 fresh processes per candidate and lease, rounds interleaved with the previous build):
    //   previous build: two process modes, fast 0.2030-0.2066 (median F = 0.2049, max - min w = 0.0025 / 0.0033), slow
    //   0.2161-0.2191, mean over all P = 0.2105 / 0.2112 -- in-step backward launch 99.9-100.3 us or 109.2-109.6 us
    //   layout  -1: 0.2050-0.2204 (same two modes)     0: 0.2018-0.2134     2: 0.2087-0.2230 (every process slow)
    //   layout   1: 0.2009-0.2060 / 0.2012-0.2040      3: 0.1996-0.2054 / 0.1990-0.2042
    //   layout   4: 0.2005-0.2030 / 0.1998-0.2033, median 0.2022 / 0.2023: one mode (max - min <= 2 w on both
    //               leases; 1 and 3 pass 2 w on one lease only), median below F; backward launch 99.3-100.0 us in 8 of 8
    // C3 (residue-split plan) is slower with it (0.4413-0.4630 against 0.4349-0.4432), C5 (two rounds, two write-back rows)
    // the same within noise (0.4830-0.4884 against 0.4840-0.4897): both keep -1.
    int lay = (dir ? o_st_layout_bwd : o_st_layout_fwd).load();
    if (lay < -1) lay = p.nsplit == 1 && mib <= 320 ? 4 : -1;
    store_layout(a, lay);
  }
  a.nsplit = p.nsplit; a.lc = p.lc;
  a.sum_in_f = p.nb == 1 && p.nsplit <= 64;       // one band: k_split_f sums the chunk partials itself (no k_split_sum)
  a.ws_z = (cf*)(ws + w.z);
  a.ws_zs = (cf*)(ws + w.zs);
  a.ws_s = (cf*)(ws + w.s);
  return a;
}

// dropout parameters of one call: thr = round(p * 65536) (0 = off)
struct DropCfg { unsigned thr = 0; float scale = 1.f; const unsigned long long* rng = nullptr; };
int drop_cfg(float p, const void* rng_state, DropCfg* out) {
  if (!(p >= 0.f) || p >= 1.f) return fail(SMX_ERR_INVALID, "dropout p must be in [0, 1), got %g", (double)p);
  long thr = lroundf(p * 65536.f);
  if (thr > 65535) thr = 65535;
  if (thr <= 0) return SMX_OK;
  if (!rng_state) return fail(SMX_ERR_INVALID, "rng_state is NULL with dropout p > 0");
  if ((uintptr_t)rng_state & 7) return fail(SMX_ERR_INVALID, "rng_state must be 8-byte aligned");
  out->thr = (unsigned)thr;
  out->scale = 65536.f / (float)(65536 - thr);
  out->rng = (const unsigned long long*)rng_state;
  return SMX_OK;
}
void set_drop(DecimArgs& a, const DropCfg& dc) { a.drop_thr = dc.thr; a.drop_scale = dc.scale; a.rng = dc.rng; }
hipError_t drop_rows(const float* in, float* out, const Shape& h, const DropCfg& dc, hipStream_t s) {
  return launch_dropout_rows(in, out, h.B, (long long)h.N * h.D, dc.thr, dc.scale, dc.rng, s);
}

// ---- steps the entries share ---------------------------------------------------------------------------------------
// the filter of a forward launch (xk_save: where the spectrum is kept for backward, or NULL) ...
void filter_fwd(DecimArgs& a, const float* w_re, const float* w_im, const float* bias, int conj_w, float* xk_save) {
  a.fa.w_re = w_re; a.fa.w_im = w_im; a.fa.bias = bias; a.fa.conj_w = conj_w;
  a.fa.xk_out = xk_save;
}
// ... and of a backward launch: conj(W), the saved spectrum, the per-batch-row products and bias partials
void filter_bwd(DecimArgs& a, const float* w_re, const float* w_im, const float* xk, char* ws, const Ws& w) {
  a.fa.w_re = w_re; a.fa.w_im = w_im; a.fa.conj_w = 1;
  a.fa.xk_in = xk; a.fa.pslab = (float*)(ws + w.slab); a.fa.gb_part = (float*)(ws + w.gbp);
}
// four-step launches: the tile spectra at `tiles`, walked in the plan's chunks
void use_tiles(DecimArgs& a, const Plan& p, void* tiles) { a.ws_f = (cf*)tiles; a.nsplit = p.fs_nsplit; a.lc = p.fs_lc; }
// the same launch without its inverse half: products out, spectrum parked
DecimArgs no_out(DecimArgs a) { a.out = nullptr; return a; }

// The filter in the layout of the unpack phase (FilterArgs::wt).  `ready`: a copy packed by an earlier
// call with the same weights (backward reusing forward's) -- nothing is launched.  `keep`: caller buffer
// that receives the packed copy.  Otherwise it goes to the workspace, and without a workspace (allowed
// for the single-launch forward) the kernels gather from (D,F) directly.
int pack_filter(DecimArgs& a, const Plan& p, const Ws& w, void* workspace, size_t workspace_bytes,
                const float* w_re, const float* w_im, int D, int F, const float* ready, float* keep,
                hipStream_t s) {
  a.fa.wt = nullptr;
  if (((uintptr_t)ready | (uintptr_t)keep) & 15)
    return fail(SMX_ERR_INVALID, "filter_pack must be 16-byte aligned");
  // Small problems are launch-latency-bound: the extra 5 us launch costs more than the gathers it saves
  // ((8,512,256): 22 -> 17 us per forward).  The rule depends on the shape only, so a forward / backward
  // pair always agrees on whether filter_pack holds anything.
  if ((double)a.g.B * a.g.R * a.g.D < 8.0 * (1 << 20)) return SMX_OK;
  // One band: every workgroup (k_fused<1, .>, k_split_f<1, .>) stages its own slice of (D,F) through LDS
  // (prefetch_w / stage_w in smx_core.h); no packed copy is read or written on either plan.
  if (p.nb == 1 && p.groups == 1) return SMX_OK;
  if (ready) { a.fa.wt = ready; return SMX_OK; }
  cf* wt = (cf*)keep;
  if (!wt) {
    if (!ws_usable(workspace, workspace_bytes, w.total)) return SMX_OK;
    wt = (cf*)((char*)workspace + w.wt);
  }
  HIP_TRY(launch_pack_w(w_re, w_im, wt, D, F, p.k, s));
  a.fa.wt = (const float*)wt;
  return SMX_OK;
}

// ---- k > 512: band groups (see make_plan) --------------------------------------------------------
// Point `a` at band group g: its residue-twiddle table, bin offset, parked-spectrum slot; only the
// first group stores (the others add) and carries the bias.
int set_group(DecimArgs& a, const Plan& p, const Tables& t, const Ws& w, char* ws, int N, int g,
              const float* bias, hipStream_t s) {
  a.bt = t.bt;
  if (g > 0) if (int rc = get_group_bt(N, g, const_cast<cf**>(&a.bt), s)) return rc;
  a.fa.goff = 512 * g;
  a.fa.multi = p.groups > 1;
  a.fa.bias = g == 0 ? bias : nullptr;
  a.accumulate = g > 0;
  a.ws_s = (cf*)(ws + w.s + (size_t)g * w.s_group);
  return SMX_OK;
}

// the bins 512, 1024, ... < k of a multi-group plan, through the literal-DFT kernels
DirectArgs edge_args(const Plan& p, const Tables& t, const Shape& h) {
  DirectArgs e{h.B, h.N, h.D, h.F, p.nedge, t.tw};
  e.f0 = 512; e.fstep = 512;
  e.R = h.R;
  return e;
}
DirectArgs direct_args(const Plan& p, const Tables& t, const Shape& h) {
  DirectArgs d{h.B, h.N, h.D, h.F, p.k, t.tw};
  d.R = h.R;
  return d;
}

}  // namespace

extern "C" {

int smx_version(void) { return SMX_VERSION; }

__global__ void k_diag_clock(unsigned long long* out2, int spin) {
  const unsigned long long c0 = clock64(), r0 = wall_clock64();       // s_memtime / s_memrealtime
  float a = (float)threadIdx.x, b = 1.0000001f;
  for (int i = 0; i < spin; ++i) a = __builtin_fmaf(a, b, 1e-7f);
  const unsigned long long c1 = clock64(), r1 = wall_clock64();
  if (threadIdx.x == 0) { out2[0] = c1 - c0; out2[1] = r1 - r0; }
  if (a == 12345.678f) out2[1] = 0;                                    // keeps the chain alive
}
int smx_diag_clock(unsigned long long* out2, int spin, void* stream) {
  if (!out2 || spin <= 0) return fail(SMX_ERR_INVALID, "out2 must be non-NULL and spin positive");
  hipLaunchKernelGGL(k_diag_clock, dim3(1), dim3(64), 0, (hipStream_t)stream, out2, spin);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}
const char* smx_last_error(void) { return t_err.c_str(); }

int smx_set_option(const char* name, int value) {
  if (!name) return fail(SMX_ERR_INVALID, "option name is NULL");
  std::atomic<int>* o = nullptr;
  if (!strcmp(name, "nsplit")) o = &o_nsplit;
  else if (!strcmp(name, "placement") || !strcmp(name, "stagger")) o = &o_placement;
  else if (!strcmp(name, "round")) o = &o_round;
  else if (!strcmp(name, "force_direct")) o = &o_force_direct;
  else if (!strcmp(name, "full8")) o = &o_full8;
  else if (!strcmp(name, "fourstep")) o = &o_fourstep;
  else if (!strcmp(name, "fs_bgroups")) o = &o_fs_bgroups;
  else if (!strcmp(name, "fold_gradw")) o = &o_fold_gradw;
  else if (!strcmp(name, "decim16")) o = &o_decim16;
  else if (!strcmp(name, "conv1")) o = &o_conv1;
  else if (!strcmp(name, "st_plain")) o = &o_st_plain;
  else if (!strcmp(name, "st_layout")) { o_st_layout_fwd = value; o = &o_st_layout_bwd; }
  else if (!strcmp(name, "st_layout_fwd")) o = &o_st_layout_fwd;
  else if (!strcmp(name, "st_layout_bwd")) o = &o_st_layout_bwd;
  else if (!strcmp(name, "tiled_dft")) { set_tiled_dft(value); g_opt_epoch++; return SMX_OK; }
  else if (!strcmp(name, "table_cache_entries")) { o_table_cap = value < 1 ? 1 : value; return SMX_OK; }
  else return fail(SMX_ERR_INVALID, "unknown option '%s'", name);
  *o = value;
  g_opt_epoch++;
  return SMX_OK;
}

int smx_options_default(smx_options* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  *out = default_opts();
  return SMX_OK;
}
int smx_options_push(const smx_options* opts) {
  if (!opts) return fail(SMX_ERR_INVALID, "opts is NULL");
  if (t_opt_depth >= OPT_DEPTH) return fail(SMX_ERR_INVALID, "smx_options_push nested deeper than %d", OPT_DEPTH);
  t_opt_stack[t_opt_depth++] = *opts;
  return SMX_OK;
}
int smx_options_pop(void) {
  if (t_opt_depth <= 0) return fail(SMX_ERR_INVALID, "smx_options_pop without a matching push");
  --t_opt_depth;
  return SMX_OK;
}
unsigned long long smx_options_epoch(void) { return g_opt_epoch.load(); }
unsigned long long smx_tables_epoch(void) { return g_tab_epoch.load(); }

// Compile-time switches this binary was built with that change what the kernels compute or how they are tuned.
// "SMX_AB_*" are timing ablations (tools/ab.sh) that return WRONG RESULTS by design: the Python loader refuses
// such a library (tensor_cuda_fft_amd._lib.load).
const char* smx_build_flags(void) {
  return ""
#ifdef SMX_AB_NO_FWD
         " SMX_AB_NO_FWD"
#endif
#ifdef SMX_AB_NO_UNPACK
         " SMX_AB_NO_UNPACK"
#endif
#ifdef SMX_AB_NO_INV
         " SMX_AB_NO_INV"
#endif
#if !SMX_NT_LOAD
         " SMX_NT_LOAD=0"
#endif
#if !SMX_NT_STORE
         " SMX_NT_STORE=0"
#endif
#ifdef SMX_BUILD_NOTE
         " " SMX_BUILD_NOTE
#endif
      ;
}

static int plan_query_impl(const Shape& h, smx_plan* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  Plan p = make_plan(h);
  out->path = p.path; out->k = p.k; out->L = p.L; out->bands = p.full8() ? 8 : p.fs() ? 0 : p.nb;
  out->nsplit = p.fs() ? p.fs_nsplit : p.nsplit;
  out->workgroups = p.path != SMX_PATH_DIRECT ? p.nwg * out->nsplit : 0;
  out->groups = p.groups_only() ? p.groups : 1;
  return SMX_OK;
}
int smx_plan_query(int B, int N, int D, int F, smx_plan* out) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  return plan_query_impl(layer_shape(B, N, D, F), out);
}
int smx_plan_query_ex(const smx_shape* shape, smx_plan* out) {
  Shape h;
  if (int rc = shape_from(shape, &h)) return rc;
  return plan_query_impl(h, out);
}

int smx_workspace_bytes(int B, int N, int D, int F, size_t* out) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  const Shape h = layer_shape(B, N, D, F);
  *out = ws_layout(make_plan(h), B, N, D).total;
  return SMX_OK;
}
int smx_workspace_bytes_ex(const smx_shape* shape, size_t* out) {
  Shape h;
  if (int rc = shape_from(shape, &h)) return rc;
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  *out = ws_layout(make_plan(h), h.B, h.N, h.D).total;
  return SMX_OK;
}

int smx_prepare(int N) {
  if (N <= 0) return fail(SMX_ERR_INVALID, "N must be positive");
  TableRef t;
  return get_tables(N, &t, nullptr);
}

static int io_check(int io) {
  if (io != SMX_IO_F32 && io != SMX_IO_BF16 && io != SMX_IO_F16)
    return fail(SMX_ERR_INVALID, "io must be SMX_IO_F32, SMX_IO_BF16 or SMX_IO_F16, got %d", io);
  return SMX_OK;
}

int smx_row_scale_supported(const smx_shape* shape) {
  Shape h;
  if (shape_from(shape, &h)) return 0;
  return make_plan(h).row_scale() ? 1 : 0;
}

// io (forward_impl, backward_impl): element type of x / y / g / grad_x, SMX_IO_*.  2-byte rows travel behind the
// float pointers and are only read by the IO instances of k_fused / k_split_a / k_split_b, on the plans of
// Plan::io_native.
static int forward_impl(const Shape& h, const float* x, const float* w_re, const float* w_im,
                        const float* bias, float* y, float* xk_save, void* workspace,
                        size_t workspace_bytes, int conj_w, float dropout_p, const void* rng_state,
                        float* filter_pack, void* stream, const float* row_scale, int io) {
  const int B = h.B, N = h.N, D = h.D, F = h.F;
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  const bool pack_ready = (conj_w & SMX_FILTER_PACK_READY) != 0;      // filter_pack already holds W
  conj_w &= 1;
  if (pack_ready && !filter_pack) return fail(SMX_ERR_INVALID, "SMX_FILTER_PACK_READY without filter_pack");
  if (!x || !w_re || !w_im || !y) return fail(SMX_ERR_INVALID, "x, w_re, w_im, y must be non-NULL");
  if (io != SMX_IO_F32) {
    if (((uintptr_t)x | (uintptr_t)y) & 3) return fail(SMX_ERR_INVALID, "2-byte x and y must be 4-byte aligned");
  } else if (((uintptr_t)x | (uintptr_t)y) & 7) return fail(SMX_ERR_INVALID, "x and y must be 8-byte aligned");
  if ((uintptr_t)xk_save & 15) return fail(SMX_ERR_INVALID, "xk_save must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Plan p = make_plan(h);
  if (io != SMX_IO_F32 && !p.io_native())
    return fail(SMX_ERR_UNSUPPORTED, "no 2-byte I/O on this plan (smx_io_supported): widen the input and call "
                "smx_forward_dropout");
  if (dc.thr && h.R < N) return fail(SMX_ERR_UNSUPPORTED, "fused dropout is not available with zero-padded rows");
  const Ws w = ws_layout(p, B, N, D);
  // (smx_forward_io has always looked at the workspace before the tables; the f32 entries look below, after them)
  if (io != SMX_IO_F32 && p.nsplit > 1) if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
  TableRef t;
  if (int rc = get_tables(N, &t, s)) return rc;
  char* ws = (char*)workspace;
  // (the sixteen-row kernels take no row scale: such a call is left to the DFT products, which refuse it)
  const bool direct = p.kind == Kind::Direct || (p.kind == Kind::Sixteen && row_scale);
  // More than 512 bins (four-step, eight-band and band-group plans): their tile stores have no fused mask, nor has the
  // direct plan; the same mask -- a pure function of (generator state, batch row, element) -- goes on y in one more pass.
  const bool post_drop = dc.thr && (p.wide() || direct);
  if (direct) {
    if (row_scale) return fail(SMX_ERR_UNSUPPORTED, "row_scale is not available on the direct plan (smx_row_scale_supported)");
    if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
    DirectArgs d = direct_args(p, t, h);
    cf* xk = xk_save ? (cf*)xk_save : (cf*)(ws + w.spec0);
    cf* sk = (cf*)(ws + w.spec1);
    HIP_TRY(launch_direct_spectrum(x, xk, d, s));
    HIP_TRY(launch_direct_filter(xk, w_re, w_im, conj_w, sk, d, s));
    HIP_TRY(launch_direct_synth(sk, bias, y, d, s));
  } else {
    if (p.kind == Kind::Split) if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
    DecimArgs a = decim_args(p, t, h, ws, w, io != SMX_IO_F32 ? 2 : 4);
    a.in = x; a.out = y;
    filter_fwd(a, w_re, w_im, bias, conj_w, xk_save);
    a.fa.sc = row_scale;
    if (row_scale && !p.row_scale())
      return fail(SMX_ERR_UNSUPPORTED, "row_scale is not available on the band-group plan (smx_row_scale_supported)");
    set_drop(a, post_drop ? DropCfg{} : dc);
    if (int rc = pack_filter(a, p, w, workspace, workspace_bytes, w_re, w_im, D, F,
                             pack_ready ? filter_pack : nullptr, pack_ready ? nullptr : filter_pack, s))
      return rc;
    if (p.kind == Kind::Sixteen) {
      if (p.nsplit == 1) {
        HIP_TRY(launch_fused16(a, p.nb, 0, s));
      } else {
        if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
        HIP_TRY(launch_split16_a(a, p.nb, false, s));
        HIP_TRY(launch_split_f(a, p.nb, 0, s));
        HIP_TRY(launch_split16_b(a, p.nb, true, s));
      }
    } else if (p.fs()) {
      if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
      use_tiles(a, p, ws + w.fs);
      HIP_TRY(launch_fs_a(a, s));
      HIP_TRY(launch_fs_f(a, 0, s));
      HIP_TRY(launch_fs_b(a, s));
    } else if (p.full8()) {
      if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
      HIP_TRY(launch_full8(a, 0, s));
    } else if (p.groups_only()) {
      if (x == y) return fail(SMX_ERR_INVALID, "the band-group plan cannot transform in place (y must not alias x)");
      if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
      for (int g = 0; g < p.groups; ++g) {
        if (int rc = set_group(a, p, t, w, ws, N, g, bias, s)) return rc;
        HIP_TRY(launch_fused(a, 4, 0, s));
      }
      DirectArgs e = edge_args(p, t, h);
      cf* xe = xk_save ? (cf*)xk_save : (cf*)(ws + w.edge0);
      e.rows = xk_save ? p.k : 0;
      HIP_TRY(launch_edge_spectrum(x, xe, (double*)(ws + w.edgep), e, s));
      HIP_TRY(launch_direct_filter(xe, w_re, w_im, conj_w, (cf*)(ws + w.edge1), e, s));
      e.rows = 0;
      HIP_TRY(launch_edge_synth_acc((cf*)(ws + w.edge1), y, e, s));
    } else if (p.kind == Kind::Single) {
      HIP_TRY(launch_fused(a, p.nb, 0, s, io));
    } else {
      HIP_TRY(launch_split_a(a, p.nb, false, s, io));
      HIP_TRY(launch_split_f(a, p.nb, 0, s));
      HIP_TRY(launch_split_b(a, p.nb, true, s, io));
    }
  }
  if (post_drop) HIP_TRY(drop_rows(y, y, h, dc, s));
  return SMX_OK;
}

int smx_forward_dropout(const float* x, const float* w_re, const float* w_im, const float* bias,
                        float* y, float* xk_save, void* workspace, size_t workspace_bytes, int B,
                        int N, int D, int F, int conj_w, float dropout_p, const void* rng_state,
                        float* filter_pack, void* stream) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  return forward_impl(layer_shape(B, N, D, F), x, w_re, w_im, bias, y, xk_save, workspace, workspace_bytes,
                      conj_w, dropout_p, rng_state, filter_pack, stream, nullptr, SMX_IO_F32);
}
int smx_forward(const float* x, const float* w_re, const float* w_im, const float* bias, float* y,
                float* xk_save, void* workspace, size_t workspace_bytes, int B, int N, int D, int F,
                int conj_w, void* stream) {
  return smx_forward_dropout(x, w_re, w_im, bias, y, xk_save, workspace, workspace_bytes, B, N, D, F,
                             conj_w, 0.f, nullptr, nullptr, stream);
}
int smx_forward_ex(const smx_shape* shape, const float* x, const float* w_re, const float* w_im,
                   const float* bias, float* y, float* xk_save, void* workspace, size_t workspace_bytes,
                   int conj_w, float* filter_pack, const float* row_scale, void* stream) {
  Shape h;
  if (int rc = shape_from(shape, &h)) return rc;
  return forward_impl(h, x, w_re, w_im, bias, y, xk_save, workspace, workspace_bytes, conj_w, 0.f, nullptr,
                      filter_pack, stream, row_scale, SMX_IO_F32);
}

static int backward_impl(const Shape& h, const float* g, const float* xk, const float* w_re,
                         const float* w_im, float* grad_x, float* gw_re, float* gw_im, float* gbias,
                         void* workspace, size_t workspace_bytes, int phases, float dropout_p,
                         const void* rng_state, const float* filter_pack, void* stream,
                         const float* row_scale, float* grad_row_scale, int io, int oio) {
  // oio: element type of grad_x where it is not g's (-1: io).  The 2-byte block backward alone passes SMX_IO_F32 here:
  // its "grad_x" is grad_h, read unrounded by the LayerNorm backward.  Mode 1 then (the only such instance of k_fused).
  if (oio < 0) oio = io;
  const int B = h.B, N = h.N, D = h.D, F = h.F;
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  if (!g || !w_re || !w_im) return fail(SMX_ERR_INVALID, "g, w_re, w_im must be non-NULL");
  phases &= ~SMX_PHASE_SYNC_CLEAN;     // accepted and ignored (smx.h)
  if (phases < 1 || phases > 7) return fail(SMX_ERR_INVALID, "phases must be a combination of 1, 2, 4");
  if ((phases & SMX_PHASE_INVERSE) && !grad_x) return fail(SMX_ERR_INVALID, "grad_x is NULL");
  const bool want_w = gw_re || gw_im || gbias;
  if (want_w && !(gw_re && gw_im && gbias))
    return fail(SMX_ERR_INVALID, "gw_re, gw_im, gbias must be given together");
  if (io != SMX_IO_F32 && oio == io) {
    if (((uintptr_t)g | (uintptr_t)grad_x) & 3)
      return fail(SMX_ERR_INVALID, "2-byte g and grad_x must be 4-byte aligned");
  } else if ((((uintptr_t)g) & (io != SMX_IO_F32 ? 3 : 7)) | ((uintptr_t)grad_x & 7))
    return fail(SMX_ERR_INVALID, "g and grad_x must be 8-byte aligned");
  if ((uintptr_t)xk & 15) return fail(SMX_ERR_INVALID, "xk must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Plan p = make_plan(h);
  if (io != SMX_IO_F32 && !p.io_native())
    return fail(SMX_ERR_UNSUPPORTED, "no 2-byte I/O on this plan (smx_io_supported): widen g and call "
                "smx_backward_dropout");
  if (dc.thr && h.R < N) return fail(SMX_ERR_UNSUPPORTED, "fused dropout is not available with zero-padded rows");
  if ((want_w || dc.thr || grad_row_scale || oio != io) && !xk && p.k > 0)
    return fail(SMX_ERR_INVALID, "xk (saved spectrum) is NULL");
  if ((row_scale || grad_row_scale) && !p.row_scale())
    return fail(SMX_ERR_UNSUPPORTED, "row_scale is not available on this plan (smx_row_scale_supported)");
  if (grad_row_scale && !row_scale) return fail(SMX_ERR_INVALID, "grad_row_scale without row_scale");
  const Ws w = ws_layout(p, B, N, D);
  if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
  TableRef t;
  if (int rc = get_tables(N, &t, s)) return rc;
  char* ws = (char*)workspace;
  const bool do_spec = phases & SMX_PHASE_SPECTRUM, do_inv = phases & SMX_PHASE_INVERSE;
  const bool do_par = (phases & SMX_PHASE_PARAMS) && want_w;

  if (p.kind != Kind::Direct) {
    // (the sixteen-row launches have always been placed by the forward launches' option, "st_layout_fwd")
    DecimArgs a = decim_args(p, t, h, ws, w, oio != SMX_IO_F32 ? 2 : 4, p.kind == Kind::Sixteen ? 0 : 1);
    a.in = g; a.out = grad_x;
    filter_bwd(a, w_re, w_im, xk, ws, w);
    // mode 0 with xk_out == NULL: input gradient only (with dropout the mask goes on the LOADED tile,
    // which only the mode-1 instantiation does: use it, the products land in the workspace unused)
    const bool pre_drop = dc.thr && p.wide();      // (see below)
    const int mode = (want_w || (dc.thr && !pre_drop) || grad_row_scale || oio != io) ? 1 : 0;
    a.fa.sc = row_scale; a.fa.gsc = grad_row_scale;
    if (p.fs() && grad_row_scale) a.fa.gsc_part = (cf*)(ws + w.gscp);
    // four-step / eight-band plans: the masked upstream gradient is staged in grad_x first (their kernels read the whole
    // input column before the first store to it, so transforming grad_x in place is safe)
    set_drop(a, pre_drop ? DropCfg{} : dc);
    if (pre_drop && do_spec) {
      if (!p.groups_only()) {
        if (!grad_x) return fail(SMX_ERR_INVALID, "dropout with more than 512 bins needs grad_x as scratch");
        if (p.full8() && !do_inv) return fail(SMX_ERR_UNSUPPORTED, "dropout on the eight-band plan needs the spectrum and inverse phases in one call");
        HIP_TRY(drop_rows(g, grad_x, h, dc, s));
        a.in = grad_x;
      } else {             // band groups: the launches re-read g while grad_x accumulates -> the workspace's row copy
        HIP_TRY(drop_rows(g, (float*)(ws + w.rows), h, dc, s));
        a.in = (const float*)(ws + w.rows);
        g = a.in;          // (the edge-bin spectrum below reads g as well)
      }
    }
    if (do_spec)
      if (int rc = pack_filter(a, p, w, workspace, workspace_bytes, w_re, w_im, D, F, filter_pack,
                               nullptr, s))
        return rc;
    int slab_rows = B;          // rows of the gradient slab that launch_gradw_slab sums, always in a launch of its own
    if (p.kind == Kind::Sixteen) {
      if (do_spec) {
        if (p.nsplit > 1) {
          HIP_TRY(launch_split16_a(a, p.nb, true, s));
          HIP_TRY(launch_split_f(a, p.nb, mode, s));
          if (do_inv) HIP_TRY(launch_split16_b(a, p.nb, false, s));
        } else {                                                     // (SPECTRUM alone: products out, spectrum parked)
          HIP_TRY(launch_fused16(do_inv ? a : no_out(a), p.nb, mode, s));
        }
      } else if (do_inv) {
        HIP_TRY(launch_split16_b(a, p.nb, false, s));               // (nsplit == 1: one chunk = every tile)
      }
    } else if (p.fs()) {
      use_tiles(a, p, ws + w.fs);
      // Option "fs_bgroups" = G > 0: slab rows summed over G batch groups inside k_fs_f (a rule of the shape
      // and the option only, so that a separate SMX_PHASE_PARAMS call reads the layout the SPECTRUM call
      // wrote).  Measured at (64,1024,512), G = 8: k_gradw 71 -> 16 us, but k_fs_f<8,1> 215 -> 286 us -- one
      // thread walking 8 batch rows exposes the load latency 9216 independent workgroups hide.  Off by default.
      const int bgo = cur_opts().fs_bgroups;
      const int bg = (bgo > 0 && fs_grouped_tiles::has(p.L) && B >= 2 * bgo) ? bgo : 0;
      a.fs_bgroups = bg;
      if (bg) slab_rows = (B + (B + bg - 1) / bg - 1) / ((B + bg - 1) / bg);
      if (do_spec) {
        HIP_TRY(launch_fs_a(a, s));
        HIP_TRY(launch_fs_f(a, mode, s));
      }
      if (do_inv) HIP_TRY(launch_fs_b(a, s));
    } else if (p.full8() && do_spec && do_inv) {
      HIP_TRY(launch_full8(a, mode, s));
    } else if (p.wide()) {             // band groups, also as the phase-split form of the eight-band plan
      DirectArgs e = edge_args(p, t, h);
      cf* ge = (cf*)(ws + w.edge0);
      cf* se = (cf*)(ws + w.edge1);
      if (do_spec) {
        HIP_TRY(launch_edge_spectrum(g, ge, (double*)(ws + w.edgep), e, s));
        HIP_TRY(launch_direct_filter(ge, w_re, w_im, 1, se, e, s));
        if (want_w) HIP_TRY(launch_edge_slab((const cf*)xk, ge, (cf*)(ws + w.slab), p.k, e, s));
      }
      for (int gi = 0; gi < p.groups; ++gi) {
        if (int rc = set_group(a, p, t, w, ws, N, gi, nullptr, s)) return rc;
        if (do_spec) {
          HIP_TRY(launch_fused(do_inv ? a : no_out(a), 4, mode, s));
        } else if (do_inv) {
          HIP_TRY(launch_split_b(a, 4, false, s));
        }
      }
      if (do_inv) HIP_TRY(launch_edge_synth_acc(se, grad_x, e, s));
    } else if (do_spec && do_inv && p.kind == Kind::Single) {
      HIP_TRY(launch_fused(a, p.nb, mode, s, io, oio));
    } else {
      if (do_spec) {
        if (p.kind == Kind::Single) {          // forward half + filter in one launch, S parked in the workspace
          HIP_TRY(launch_fused(no_out(a), p.nb, mode, s, io, oio));
        } else {
          HIP_TRY(launch_split_a(a, p.nb, true, s, io));
          HIP_TRY(launch_split_f(a, p.nb, mode, s));
        }
      }
      if (do_inv) HIP_TRY(launch_split_b(a, p.nb, false, s, oio));
    }
    if (do_par)
      HIP_TRY(launch_gradw_slab((cf*)(ws + w.slab), (float*)(ws + w.gbp), gw_re, gw_im, gbias, slab_rows, D, F, p.k, s));
    return SMX_OK;
  }

  // direct path: spec0 = G (k' = max(k,1) bins so grad_bias is available when k == 0), spec1 = S
  DirectArgs d = direct_args(p, t, h);
  cf* gk = (cf*)(ws + w.spec0);
  cf* sk = (cf*)(ws + w.spec1);
  if (do_spec) {
    DirectArgs dg = d;
    if (p.k == 0) dg.k = 1;
    if (dc.thr) {            // masked upstream gradient, staged in grad_x (overwritten by the synthesis)
      if (!grad_x) return fail(SMX_ERR_INVALID, "dropout on the direct plan needs grad_x as scratch");
      HIP_TRY(drop_rows(g, grad_x, h, dc, s));
      g = grad_x;
    }
    HIP_TRY(launch_direct_spectrum(g, gk, dg, s));
    HIP_TRY(launch_direct_filter(gk, w_re, w_im, 1, sk, d, s));
  }
  if (do_par) {
    if (p.k == 0) {
      HIP_TRY(hipMemsetAsync(gw_re, 0, (size_t)D * F * sizeof(float), s));
      HIP_TRY(hipMemsetAsync(gw_im, 0, (size_t)D * F * sizeof(float), s));
      // grad_bias = sum_b G[b,0,d].re : reuse the reduction with one bin and a dummy X
      // (its weight-gradient outputs go to spec2, which nothing else uses)
      float* scratch = (float*)(ws + w.spec2);
      HIP_TRY(launch_gradw_spectra(gk, gk, scratch, scratch + D, gbias, B, N, D, 1, 1, s));
    } else {
      HIP_TRY(launch_gradw_spectra((const cf*)xk, gk, gw_re, gw_im, gbias, B, N, D, F, p.k, s));
    }
  }
  if (do_inv) HIP_TRY(launch_direct_synth(sk, nullptr, grad_x, d, s));
  return SMX_OK;
}

int smx_backward_dropout(const float* g, const float* xk, const float* w_re, const float* w_im,
                         float* grad_x, float* gw_re, float* gw_im, float* gbias, void* workspace,
                         size_t workspace_bytes, int B, int N, int D, int F, int phases,
                         float dropout_p, const void* rng_state, const float* filter_pack,
                         void* stream) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  return backward_impl(layer_shape(B, N, D, F), g, xk, w_re, w_im, grad_x, gw_re, gw_im, gbias, workspace,
                       workspace_bytes, phases, dropout_p, rng_state, filter_pack, stream, nullptr, nullptr,
                       SMX_IO_F32, -1);
}
int smx_backward(const float* g, const float* xk, const float* w_re, const float* w_im,
                 float* grad_x, float* gw_re, float* gw_im, float* gbias, void* workspace,
                 size_t workspace_bytes, int B, int N, int D, int F, int phases, void* stream) {
  return smx_backward_dropout(g, xk, w_re, w_im, grad_x, gw_re, gw_im, gbias, workspace,
                              workspace_bytes, B, N, D, F, phases, 0.f, nullptr, nullptr, stream);
}
int smx_backward_ex(const smx_shape* shape, const float* g, const float* xk, const float* w_re,
                    const float* w_im, float* grad_x, float* gw_re, float* gw_im, float* gbias,
                    void* workspace, size_t workspace_bytes, int phases, const float* filter_pack,
                    const float* row_scale, float* grad_row_scale, void* stream) {
  Shape h;
  if (int rc = shape_from(shape, &h)) return rc;
  return backward_impl(h, g, xk, w_re, w_im, grad_x, gw_re, gw_im, gbias, workspace, workspace_bytes, phases,
                       0.f, nullptr, filter_pack, stream, row_scale, grad_row_scale, SMX_IO_F32, -1);
}

// complex sequence FFT: (A) tile spectra + (F) columns written straight out; its own plan (any L the column
// kernel is instantiated for, also below the 512-bin threshold of the filter plans)
static bool cfft_plan(const Shape& h, Plan* p) {
  if (h.N % M != 0 || h.D % 2 != 0 || h.R > h.N || !fs_tiles_cfft(h.N / M)) return false;
  *p = tile_plan(h);
  return true;
}
static size_t cfft_need(const Plan& p) { return WS_HEADER_BYTES + al((size_t)p.nwg * p.L * EX * sizeof(cf)); }   // behind the reserved header (ws_layout)
int smx_cfft_workspace_bytes(const smx_shape* shape, size_t* out) {
  if (!shape || !out) return fail(SMX_ERR_INVALID, "NULL argument");
  Shape h{shape->B, shape->rows, shape->D, shape->n_fft / 2 + 1, shape->n_fft, shape->n_fft / 2 + 1};
  if (int rc = check_shape(h)) return rc;
  Plan p;
  if (!cfft_plan(h, &p)) return fail(SMX_ERR_UNSUPPORTED, "smx_cfft_ex does not take this shape");
  *out = cfft_need(p);
  return SMX_OK;
}
int smx_cfft_ex(const smx_shape* shape, const float* z, float* out, void* workspace, size_t workspace_bytes,
                void* stream) {
  if (!shape) return fail(SMX_ERR_INVALID, "shape is NULL");
  Shape h{shape->B, shape->rows, shape->D, shape->n_fft / 2 + 1, shape->n_fft, shape->n_fft / 2 + 1};
  if (int rc = check_shape(h)) return rc;
  if (!z || !out) return fail(SMX_ERR_INVALID, "z and out must be non-NULL");
  if (((uintptr_t)z | (uintptr_t)out) & 7) return fail(SMX_ERR_INVALID, "z and out must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  Plan p;
  if (!cfft_plan(h, &p))
    return fail(SMX_ERR_UNSUPPORTED, "smx_cfft_ex needs n_fft = 256 L with L in {2, 4, 5..32, 36..64 step 4, 72..128 step 8, 144..256 step 16} and an even D; "
                                     "compose it from smx_spectrum_ex otherwise");
  if (int rc = need_ws(workspace, workspace_bytes, cfft_need(p), "smx_cfft_workspace_bytes")) return rc;
  TableRef t;
  if (int rc = get_tables(h.N, &t, s)) return rc;
  Ws dummy;
  DecimArgs a = decim_args(p, t, h, (char*)workspace, dummy);
  a.ws_z = a.ws_zs = a.ws_s = nullptr;
  a.in = z; a.out = nullptr;
  a.fa.xk_out = out;
  use_tiles(a, p, (char*)workspace + WS_HEADER_BYTES);
  HIP_TRY(launch_fs_a(a, s));
  HIP_TRY(launch_fs_f(a, 3, s));
  return SMX_OK;
}

// ---- rank-one filter: the causal FFT convolution of fft_lm on the four-step path ------------------------
namespace {
struct ConvWs { size_t fs = 0, pp = 0, rp = 0, total = 0, save = 0; };
static bool conv_plan(const Shape& h, Plan* p) {
  // its own plan: tile spectra / columns / inverse tiles for n_fft = 512 ... 65536 (four columns of L values each
  // fit one thread's registers in backward up to L = 16; above that L / 16 threads share a column pair)
  if (h.N % M != 0 || h.D % 2 != 0 || h.R > h.N || !conv_tiles(h.N / M)) return false;
  *p = tile_plan(h);
  // One launch per direction where the zero padding allows it (k_conv1).  Its workgroup owns 32 channels (512 threads,
  // one per CU) or 16 (256 threads, two per CU, 64-byte row segments); measured, hipGraph fwd+bwd at n_fft 2048
  // (profiles/r03_f2_conv1_ab.txt), by the count w of (batch row, 32-channel tile) items:
  //   w = 16: 0.061 ms three launches / 0.078 / 0.069    w = 64: 0.089 / 0.093 / 0.084     w = 128: 0.116 / 0.098 / 0.090
  //   w = 256: 0.182 / 0.114 / 0.108                     w = 512:   -   / 0.186 / 0.181    w = 1024: 0.663 / 0.350 / 0.367
  // so: below 48 items the three launches (they cut the residues into chunks to fill the chip), up to 768 the
  // 16-channel workgroups, above that the 32-channel ones.
  // Option "conv1": 1 = that rule (default), 0 = never, 2 / 3 = wherever the shape allows it with 32- / 16-channel
  // workgroups.
  const int c1 = cur_opts().conv1;
  p->conv1 = c1 != 0 && conv1_supported(h.N, h.R) && (c1 >= 2 || p->nwg >= 48);
  p->conv1_nj = c1 == 3 ? 8 : c1 == 2 ? 16 : (p->nwg <= 768 ? 8 : 16);
  return true;
}
static ConvWs conv_ws(const Plan& p, const Shape& h) {
  ConvWs w;
  size_t o = WS_HEADER_BYTES;     // as every layout: the first 64 KiB are reserved and unused (ws_layout)
  w.save = (size_t)p.nwg * p.L * EX * sizeof(cf);      // (k_conv1: [workgroup][16 L / 2][512], the same bytes;
  if (p.conv1 && p.conv1_nj == 8)                       //  on 16-channel workgroups a ragged last tile rounds up)
    w.save = (size_t)conv1_workgroups(h.B, h.D, 8) * (p.L / 2 * 16) * 256 * sizeof(cf);
  w.fs = o; o += p.conv1 ? 0 : al(w.save);              // tile spectra in flight: the three-launch form only
  const size_t nwg = p.conv1 ? (size_t)conv1_workgroups(h.B, h.D, p.conv1_nj) : (size_t)p.nwg;
  w.pp = o; o += al((nwg + 32) * h.N * sizeof(cf));                 // partials (+ 32 spare rows: the staging area of the former two-stage sum)
  w.rp = o; o += al((size_t)p.nwg * conv_column_blocks(p.L) * 16 * sizeof(cf));
  w.total = o;
  return w;
}
const char* const CONV_SHAPES = "smx_conv_* needs n_fft = 512 ... 65536 (a power of two), rows <= n_fft and an even "
                                 "channel count";
int conv_shape(const smx_shape* sh, Shape* h) {
  if (!sh) return fail(SMX_ERR_INVALID, "shape is NULL");
  *h = Shape{sh->B, sh->rows, sh->D, sh->n_fft / 2 + 1, sh->n_fft, sh->n_fft / 2 + 1};
  return check_shape(*h);
}
}  // namespace

int smx_conv_supported(const smx_shape* shape) {
  Shape h; Plan p;
  if (conv_shape(shape, &h)) return 0;
  return conv_plan(h, &p) ? 1 : 0;
}
int smx_conv_workspace_bytes(const smx_shape* shape, size_t* workspace_bytes, size_t* save_bytes) {
  Shape h; Plan p;
  if (int rc = conv_shape(shape, &h)) return rc;
  if (!conv_plan(h, &p)) return fail(SMX_ERR_UNSUPPORTED, CONV_SHAPES);
  const ConvWs w = conv_ws(p, h);
  if (workspace_bytes) *workspace_bytes = w.total;
  if (save_bytes) *save_bytes = w.save;
  return SMX_OK;
}

// t: the caller's TableRef -- the tables stay pinned until the entry point has enqueued its launches
// elem: bytes per element of x / y / g / grad_x (4; 2 for 2-byte rows, conv_forward_impl / conv_backward_impl)
static int conv_args(const Shape& h, const Plan& p, const ConvWs& w, void* workspace, size_t workspace_bytes,
                     const float* h_re, const float* h_im, const float* row_scale, hipStream_t s, TableRef& t,
                     DecimArgs* out, int elem) {
  if (int rc = need_ws(workspace, workspace_bytes, w.total, "")) return rc;
  if (!h_re || !h_im) return fail(SMX_ERR_INVALID, "h_re, h_im must be non-NULL");
  if (int rc = get_tables(h.N, &t, s)) return rc;
  Ws dummy;
  DecimArgs a = decim_args(p, t, h, (char*)workspace, dummy, elem);
  a.ws_z = a.ws_zs = a.ws_s = nullptr;
  use_tiles(a, p, (char*)workspace + w.fs);
  a.ca.h_re = h_re; a.ca.h_im = h_im; a.ca.sc = row_scale;
  a.ca.p_part = (cf*)((char*)workspace + w.pp);
  a.ca.r_part = (cf*)((char*)workspace + w.rp);
  a.out_scale = row_scale;
  *out = a;
  return SMX_OK;
}

static const char* const CONV_IO_PLANS = "no 2-byte I/O on this plan (smx_conv_io_supported: the single-launch plan, "
                                         "n_fft <= 2048): widen the input and call the f32 entry";

// io: element type of x / y (g / grad_x), SMX_IO_*; 2-byte rows travel behind the float pointers and are read by
// k_conv1's IO instances only
static int conv_forward_impl(const smx_shape* shape, const float* x, const float* h_re, const float* h_im,
                             const float* row_scale, float* y, float* x_spectra, void* workspace,
                             size_t workspace_bytes, int io, void* stream) {
  Shape h; Plan p;
  if (int rc = conv_shape(shape, &h)) return rc;
  if (!conv_plan(h, &p)) return fail(SMX_ERR_UNSUPPORTED, CONV_SHAPES);
  if (io != SMX_IO_F32 && !p.conv1) return fail(SMX_ERR_UNSUPPORTED, "%s", CONV_IO_PLANS);
  if (!x || !y) return fail(SMX_ERR_INVALID, "x and y must be non-NULL");
  if (io != SMX_IO_F32) {
    if (((uintptr_t)x | (uintptr_t)y) & 3) return fail(SMX_ERR_INVALID, "2-byte x and y must be 4-byte aligned");
    if ((uintptr_t)x_spectra & 7) return fail(SMX_ERR_INVALID, "x_spectra must be 8-byte aligned");
  } else if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)x_spectra) & 7)
    return fail(SMX_ERR_INVALID, "x, y, x_spectra must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const ConvWs w = conv_ws(p, h);
  DecimArgs a;
  TableRef t;
  if (int rc = conv_args(h, p, w, workspace, workspace_bytes, h_re, h_im, row_scale, s, t, &a, io != SMX_IO_F32 ? 2 : 4))
    return rc;
  a.in = x; a.out = y;
  if (p.conv1) {
    a.ws_f = (cf*)x_spectra;                        // packed spectrum of x for backward, or NULL (inference)
    HIP_TRY(launch_conv1(a, p.conv1_nj, 0, nullptr, nullptr, nullptr, s, io));
    return SMX_OK;
  }
  cf* filtered = a.ws_f;
  if (x_spectra) a.ws_f = (cf*)x_spectra;           // (A) writes the tile spectra of x where backward finds them
  HIP_TRY(launch_fs_a(a, s));
  a.conv_src = a.ws_f;
  a.ws_f = filtered;
  HIP_TRY(launch_fs_conv(a, 0, nullptr, nullptr, nullptr, s));
  HIP_TRY(launch_fs_b(a, s));
  return SMX_OK;
}
int smx_conv_forward(const smx_shape* shape, const float* x, const float* h_re, const float* h_im,
                     const float* row_scale, float* y, float* x_spectra, void* workspace,
                     size_t workspace_bytes, void* stream) {
  return conv_forward_impl(shape, x, h_re, h_im, row_scale, y, x_spectra, workspace, workspace_bytes, SMX_IO_F32,
                           stream);
}

static int conv_backward_impl(const smx_shape* shape, const float* g, const float* x_spectra, const float* h_re,
                              const float* h_im, const float* row_scale, float* grad_x, float* grad_h_re,
                              float* grad_h_im, float* grad_row_scale, void* workspace, size_t workspace_bytes,
                              int io, void* stream) {
  Shape h; Plan p;
  if (int rc = conv_shape(shape, &h)) return rc;
  if (!conv_plan(h, &p)) return fail(SMX_ERR_UNSUPPORTED, CONV_SHAPES);
  if (io != SMX_IO_F32 && !p.conv1) return fail(SMX_ERR_UNSUPPORTED, "%s", CONV_IO_PLANS);
  if (!g || !x_spectra || !grad_x) return fail(SMX_ERR_INVALID, "g, x_spectra, grad_x must be non-NULL");
  if (io != SMX_IO_F32) {
    if (((uintptr_t)g | (uintptr_t)grad_x) & 3)
      return fail(SMX_ERR_INVALID, "2-byte g and grad_x must be 4-byte aligned");
    if ((uintptr_t)x_spectra & 7) return fail(SMX_ERR_INVALID, "x_spectra must be 8-byte aligned");
  } else if (((uintptr_t)g | (uintptr_t)grad_x | (uintptr_t)x_spectra) & 7)
    return fail(SMX_ERR_INVALID, "g, grad_x, x_spectra must be 8-byte aligned");
  if ((grad_h_re == nullptr) != (grad_h_im == nullptr))
    return fail(SMX_ERR_INVALID, "grad_h_re and grad_h_im must be given together");
  hipStream_t s = (hipStream_t)stream;
  const ConvWs w = conv_ws(p, h);
  DecimArgs a;
  TableRef t;
  if (int rc = conv_args(h, p, w, workspace, workspace_bytes, h_re, h_im, row_scale, s, t, &a, io != SMX_IO_F32 ? 2 : 4))
    return rc;
  a.in = g; a.out = grad_x;
  a.ca.xs = (const cf*)x_spectra;
  if (p.conv1) {
    HIP_TRY(launch_conv1(a, p.conv1_nj, 1, grad_h_re, grad_h_im, grad_row_scale, s, io));
    return SMX_OK;
  }
  HIP_TRY(launch_fs_a(a, s));
  a.conv_src = a.ws_f;
  HIP_TRY(launch_fs_conv(a, 1, grad_h_re, grad_h_im, grad_row_scale, s));
  HIP_TRY(launch_fs_b(a, s));
  return SMX_OK;
}
int smx_conv_backward(const smx_shape* shape, const float* g, const float* x_spectra, const float* h_re,
                      const float* h_im, const float* row_scale, float* grad_x, float* grad_h_re,
                      float* grad_h_im, float* grad_row_scale, void* workspace, size_t workspace_bytes,
                      void* stream) {
  return conv_backward_impl(shape, g, x_spectra, h_re, h_im, row_scale, grad_x, grad_h_re, grad_h_im, grad_row_scale,
                            workspace, workspace_bytes, SMX_IO_F32, stream);
}

int smx_phase_filter(const float* magnitude, const float* phase, int D, int k, int n_fft, float* w_re, float* w_im,
                     void* stream) {
  if (D <= 0 || k <= 0 || n_fft <= 0 || k > n_fft / 2 + 1) return fail(SMX_ERR_INVALID, "need D > 0, 0 < k <= n_fft / 2 + 1");
  if (!magnitude || !phase || !w_re || !w_im) return fail(SMX_ERR_INVALID, "magnitude, phase, w_re, w_im must be non-NULL");
  HIP_TRY(launch_phase_filter(magnitude, phase, D, k, n_fft, w_re, w_im, (hipStream_t)stream));
  return SMX_OK;
}
int smx_phase_filter_backward(const float* magnitude, const float* phase, const float* grad_w_re, const float* grad_w_im,
                              int D, int k, int n_fft, int row_pitch, float* grad_magnitude, float* grad_phase,
                              void* stream) {
  if (D <= 0 || k <= 0 || n_fft <= 0 || k > n_fft / 2 + 1 || row_pitch < k)
    return fail(SMX_ERR_INVALID, "need D > 0, 0 < k <= n_fft / 2 + 1, row_pitch >= k");
  if (!magnitude || !phase || !grad_w_re || !grad_w_im) return fail(SMX_ERR_INVALID, "magnitude, phase, grad_w_re, grad_w_im must be non-NULL");
  HIP_TRY(launch_phase_filter_bwd(magnitude, phase, grad_w_re, grad_w_im, D, k, n_fft, row_pitch, grad_magnitude,
                                  grad_phase, (hipStream_t)stream));
  return SMX_OK;
}

int smx_conv_response(int n_fft, int taps, const float* kernel, const float* gate_logits, const float* mask,
                      float* h_re, float* h_im, void* stream) {
  if (n_fft < 2 || taps < 1 || taps > n_fft) return fail(SMX_ERR_INVALID, "need 1 <= taps <= n_fft, n_fft >= 2");
  if (!kernel || !h_re || !h_im) return fail(SMX_ERR_INVALID, "kernel, h_re, h_im must be non-NULL");
  hipStream_t s = (hipStream_t)stream;
  TableRef t;
  if (int rc = get_tables(n_fft, &t, s)) return rc;
  HIP_TRY(launch_conv_response(kernel, gate_logits, mask, t.tw, n_fft, taps, h_re, h_im, s));
  return SMX_OK;
}
int smx_conv_response_backward(int n_fft, int taps, int n_logits, const float* kernel, const float* gate_logits,
                               const float* mask, const float* grad_h_re, const float* grad_h_im, float* grad_kernel,
                               float* grad_gate_logits, void* stream) {
  if (n_fft < 2 || taps < 1 || taps > n_fft) return fail(SMX_ERR_INVALID, "need 1 <= taps <= n_fft, n_fft >= 2");
  if (!kernel || !grad_h_re || !grad_h_im) return fail(SMX_ERR_INVALID, "kernel, grad_h_re, grad_h_im must be non-NULL");
  if (grad_gate_logits && (!gate_logits || n_logits < n_fft / 2 + 1))
    return fail(SMX_ERR_INVALID, "grad_gate_logits needs gate_logits with at least n_fft / 2 + 1 entries");
  hipStream_t s = (hipStream_t)stream;
  TableRef t;
  if (int rc = get_tables(n_fft, &t, s)) return rc;
  HIP_TRY(launch_conv_response_bwd(kernel, gate_logits, mask, t.tw, n_fft, taps, n_logits, grad_h_re, grad_h_im,
                                   grad_kernel, grad_gate_logits, s));
  return SMX_OK;
}

static int spectrum_impl(const Shape& h, const float* x, float* xk, void* workspace,
                         size_t workspace_bytes, void* stream) {
  const int B = h.B, N = h.N, D = h.D;
  if (h.k == 0) return SMX_OK;
  if (!x || !xk) return fail(SMX_ERR_INVALID, "x and xk must be non-NULL");
  if ((uintptr_t)x & 7) return fail(SMX_ERR_INVALID, "x must be 8-byte aligned");
  if ((uintptr_t)xk & 15) return fail(SMX_ERR_INVALID, "xk must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Plan p = make_plan(h);
  const Ws w = ws_layout(p, B, N, D);
  TableRef t;
  if (int rc = get_tables(N, &t, s)) return rc;
  if (p.kind == Kind::Direct) {
    DirectArgs d = direct_args(p, t, h);
    HIP_TRY(launch_direct_spectrum(x, (cf*)xk, d, s));
    return SMX_OK;
  }
  if (p.nsplit > 1) if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
  DecimArgs a = decim_args(p, t, h, (char*)workspace, w);
  a.in = x; a.out = nullptr;
  // mode 2: unpack only -- no weights are read, no S is produced
  a.fa.xk_out = xk;
  a.ws_s = nullptr;                          // nothing is parked (the workspace may be absent altogether)
  if (p.kind == Kind::Sixteen) {
    if (p.nsplit == 1) {
      HIP_TRY(launch_fused16(a, p.nb, 2, s));
    } else {
      HIP_TRY(launch_split16_a(a, p.nb, false, s));
      HIP_TRY(launch_split_f(a, p.nb, 2, s));
    }
  } else if (p.fs()) {
    if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
    use_tiles(a, p, (char*)workspace + w.fs);
    HIP_TRY(launch_fs_a(a, s));
    HIP_TRY(launch_fs_f(a, 2, s));
  } else if (p.full8()) {
    HIP_TRY(launch_full8(a, 2, s));
  } else if (p.groups_only()) {
    if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
    for (int g = 0; g < p.groups; ++g) {
      if (int rc = set_group(a, p, t, w, (char*)workspace, N, g, nullptr, s)) return rc;
      a.ws_s = nullptr;
      HIP_TRY(launch_fused(a, 4, 2, s));
    }
    DirectArgs e = edge_args(p, t, h);
    e.rows = p.k;
    HIP_TRY(launch_edge_spectrum(x, (cf*)xk, (double*)((char*)workspace + w.edgep), e, s));
  } else if (p.kind == Kind::Single) {
    HIP_TRY(launch_fused(a, p.nb, 2, s));
  } else {
    HIP_TRY(launch_split_a(a, p.nb, false, s));
    HIP_TRY(launch_split_f(a, p.nb, 2, s));
  }
  return SMX_OK;
}
int smx_spectrum(const float* x, float* xk, void* workspace, size_t workspace_bytes, int B, int N,
                 int D, int F, void* stream) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  return spectrum_impl(layer_shape(B, N, D, F), x, xk, workspace, workspace_bytes, stream);
}
int smx_spectrum_ex(const smx_shape* shape, const float* x, float* xk, void* workspace,
                    size_t workspace_bytes, void* stream) {
  Shape h;
  if (int rc = shape_from(shape, &h)) return rc;
  return spectrum_impl(h, x, xk, workspace, workspace_bytes, stream);
}

// N = 2048 with more than 512 bins (the reference's default causal-convolution length, Plan::pair8): the two halves of
// the pair run as ONE launch each with the eight bands in registers -- the tensor and the spectrum cross HBM once
// (measured at (64,1024,512): rfft 153 us against 203 us on the four-step path, which round-trips a workspace).
// These two launches touch no workspace (none is required, whatever smx_workspace_bytes_ex says for the filter
// plans of the same shape); option full8 = 0 sends the pair down the four-step path like every other length.
int smx_rfft_ex(const smx_shape* shape, const float* x, float* spec, float scale, int hermitian,
                void* workspace, size_t workspace_bytes, void* stream) {
  Shape h;
  if (int rc = shape_from(shape, &h)) return rc;
  const Plan p8 = make_plan(h);
  if (h.k > 0 && p8.pair8) {
    if (!x || !spec) return fail(SMX_ERR_INVALID, "x and spec must be non-NULL");
    if (((uintptr_t)x & 7) || ((uintptr_t)spec & 15))
      return fail(SMX_ERR_INVALID, "x must be 8-byte and spec 16-byte aligned");
    TableRef t;
    if (int rc = get_tables(h.N, &t, (hipStream_t)stream)) return rc;
    DecimArgs a = decim_args(p8, t, h, (char*)workspace, ws_layout(p8, h.B, h.N, h.D));
    a.in = x; a.out = nullptr; a.fa.xk_out = spec; a.ws_s = nullptr;
    HIP_TRY(launch_full8(a, 2, (hipStream_t)stream));
  } else if (int rc = spectrum_impl(h, x, spec, workspace, workspace_bytes, stream)) return rc;
  if (h.k > 0 && (scale != 1.f || hermitian))
    HIP_TRY(launch_scale_bins((const cf*)spec, (cf*)spec, h.B, h.k, h.D, h.N, scale, hermitian,
                              (hipStream_t)stream));
  return SMX_OK;
}

int smx_irfft_ex(const smx_shape* shape, const float* spec, float* y, float scale, int hermitian,
                 void* workspace, size_t workspace_bytes, void* stream) {
  Shape h;
  if (int rc = shape_from(shape, &h)) return rc;
  const int B = h.B, N = h.N, D = h.D;
  if (!y) return fail(SMX_ERR_INVALID, "y must be non-NULL");
  hipStream_t s = (hipStream_t)stream;
  if (h.k == 0) {
    HIP_TRY(hipMemsetAsync(y, 0, (size_t)B * h.R * D * sizeof(float), s));
    return SMX_OK;
  }
  if (!spec) return fail(SMX_ERR_INVALID, "spec must be non-NULL");
  if ((uintptr_t)y & 7) return fail(SMX_ERR_INVALID, "y must be 8-byte aligned");
  if ((uintptr_t)spec & 15) return fail(SMX_ERR_INVALID, "spec must be 16-byte aligned");
  const Plan p = make_plan(h);
  const Ws w = ws_layout(p, B, N, D);
  TableRef t;
  if (int rc = get_tables(N, &t, s)) return rc;
  char* ws = (char*)workspace;
  if (p.row_scale() || p.pair8) {      // (the kinds with synthesis kernels: up to 512 bins, four-step, the pair's eight bands)
    if (!p.pair8 && (p.fs() || p.nsplit > 1)) if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
    DecimArgs a = decim_args(p, t, h, ws, w);
    a.in = nullptr; a.out = y;
    a.fa.xk_in = spec; a.fa.sp_scale = scale; a.fa.sp_herm = hermitian;
    if (p.pair8) {
      HIP_TRY(launch_synth8(a, s));
    } else if (p.fs()) {
      use_tiles(a, p, ws + w.fs);
      HIP_TRY(launch_fs_f(a, 4, s));
      HIP_TRY(launch_fs_b(a, s));
    } else if (p.nsplit == 1) {
      HIP_TRY(launch_synth(a, p.nb, s));
    } else {
      HIP_TRY(launch_synth(no_out(a), p.nb, s));
      HIP_TRY(launch_split_b(a, p.nb, false, s));
    }
    return SMX_OK;
  }
  // DFT products: the direct plan, and the band-group plans (k > 512 at tile counts the four-step path does
  // not take) -- weighted copy of the spectrum in the workspace, then the synthesis kernels of the direct path
  if (int rc = need_ws(w, workspace, workspace_bytes)) return rc;
  cf* sk = (cf*)(ws + (p.path == SMX_PATH_DECIMATED ? w.slab : w.spec1));
  DirectArgs d = direct_args(p, t, h);
  HIP_TRY(launch_scale_bins((const cf*)spec, sk, B, p.k, D, N, scale, hermitian, s));
  HIP_TRY(launch_direct_synth(sk, nullptr, y, d, s));
  return SMX_OK;
}

int smx_grad_w(const float* xk, const float* gk, float* gw_re, float* gw_im, float* gbias, int B,
               int N, int D, int F, void* stream) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  if (!gw_re || !gw_im) return fail(SMX_ERR_INVALID, "gw_re, gw_im must be non-NULL");
  const int k = F < N / 2 ? F : N / 2;
  if (k > 0 && (!xk || !gk)) return fail(SMX_ERR_INVALID, "xk, gk must be non-NULL");
  HIP_TRY(launch_gradw_spectra((const cf*)xk, (const cf*)gk, gw_re, gw_im, gbias, B, N, D, F, k,
                               (hipStream_t)stream));
  return SMX_OK;
}

int smx_wfilter_forward(const float* x_freq, const float* w_re, const float* w_im, float* out, int B,
                        int N, int D, int F, int conj_w, void* stream) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  if (!x_freq || !w_re || !w_im || !out) return fail(SMX_ERR_INVALID, "NULL argument");
  const int k = F < N / 2 ? F : N / 2;
  HIP_TRY(launch_wfilter((const cf*)x_freq, w_re, w_im, conj_w, (cf*)out, B, N, D, F, k,
                         (hipStream_t)stream));
  return SMX_OK;
}

int smx_wfilter_grad_w(const float* x_freq, const float* g_freq, float* gw_re, float* gw_im, int B,
                       int N, int D, int F, void* stream) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  if (!x_freq || !g_freq || !gw_re || !gw_im) return fail(SMX_ERR_INVALID, "NULL argument");
  const int k = F < N / 2 ? F : N / 2;
  HIP_TRY(launch_wfilter_gradw((const cf*)x_freq, (const cf*)g_freq, gw_re, gw_im, B, N, D, F, k,
                               (hipStream_t)stream));
  return SMX_OK;
}

int smx_cmul(const float* x, const float* w, float* out, long long batch, long long inner,
             int conj_w, void* stream) {
  if (batch < 0 || inner < 0) return fail(SMX_ERR_INVALID, "negative size");
  if (batch * inner == 0) return SMX_OK;
  if (!x || !w || !out) return fail(SMX_ERR_INVALID, "NULL argument");
  HIP_TRY(launch_cmul((const cf*)x, (const cf*)w, conj_w, (cf*)out, batch, inner,
                      (hipStream_t)stream));
  return SMX_OK;
}

int smx_cmul_grad_w(const float* x, const float* g, float* gw, long long batch, long long inner,
                    void* stream) {
  if (batch < 0 || inner < 0) return fail(SMX_ERR_INVALID, "negative size");
  if (inner == 0) return SMX_OK;
  if (!x || !g || !gw) return fail(SMX_ERR_INVALID, "NULL argument");
  HIP_TRY(launch_cmul_gradw((const cf*)x, (const cf*)g, (cf*)gw, batch, inner,
                            (hipStream_t)stream));
  return SMX_OK;
}

int smx_rng_next(void* state, void* saved, void* stream) {
  if (!state || !saved) return fail(SMX_ERR_INVALID, "state and saved must be non-NULL");
  if (((uintptr_t)state | (uintptr_t)saved) & 7) return fail(SMX_ERR_INVALID, "8-byte alignment required");
  HIP_TRY(launch_rng_next((unsigned long long*)state, (unsigned long long*)saved, (hipStream_t)stream));
  return SMX_OK;
}

int smx_block_supported(int D) { return ln_supported(D) ? 1 : 0; }

// The fused block with 2-byte x / y / g / grad_x exists where k_fused_blk does -- the decimated single-launch plan --
// and where the row kernels move 2-byte chunks (ln_io_supported: D % 4 == 0).
static bool block_io_native(const Plan& p, int D) { return p.block_fused() && ln_io_supported(D); }
static const char* const BLOCK_IO_PLANS = "no 2-byte block rows on this plan (smx_block_io_supported: the decimated "
                                          "single-launch plan, D %% 4 == 0): widen the input and call the f32 entry";

// io: element type of x and y (2-byte rows behind the float pointers, as in forward_impl)
static int block_forward_impl(const float* x, const float* ln_w, const float* ln_b, float eps,
                              const float* w_re, const float* w_im, const float* bias, float* y,
                              float* xk_save, float* ln_stats, void* workspace,
                              size_t workspace_bytes, int B, int N, int D, int F, float dropout_p,
                              const void* rng_state, float* filter_pack, void* stream, int io) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  if (!ln_supported(D)) return fail(SMX_ERR_UNSUPPORTED, "LayerNorm width D=%d is not supported", D);
  const Shape h = layer_shape(B, N, D, F);
  const Plan p = make_plan(h);
  if (io != SMX_IO_F32 && !block_io_native(p, D)) return fail(SMX_ERR_UNSUPPORTED, BLOCK_IO_PLANS);
  if (!x || !w_re || !w_im || !y || !ln_stats)
    return fail(SMX_ERR_INVALID, "x, w_re, w_im, y, ln_stats must be non-NULL");
  if (x == y) return fail(SMX_ERR_INVALID, "y must not alias x");
  if (io != SMX_IO_F32) {
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)ln_stats) & 7)
      return fail(SMX_ERR_INVALID, "2-byte x and y (D %% 4 == 0) and ln_stats must be 8-byte aligned");
    if (((uintptr_t)ln_w | (uintptr_t)ln_b) & 15) return fail(SMX_ERR_INVALID, "ln_w, ln_b must be 16-byte aligned");
  } else {
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)ln_stats) & 7)
      return fail(SMX_ERR_INVALID, "x, y and ln_stats must be 8-byte aligned");
    if (D % 4 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)ln_w | (uintptr_t)ln_b) & 15))
      return fail(SMX_ERR_INVALID, "x, y, ln_w, ln_b must be 16-byte aligned");
  }
  if ((uintptr_t)xk_save & 15) return fail(SMX_ERR_INVALID, "xk_save must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long rows = (long long)B * N;
  if (io != SMX_IO_F32) HIP_TRY(launch_ln_stats_io(x, (cf*)ln_stats, rows, D, eps, s, io));
  else HIP_TRY(launch_ln_stats(x, (cf*)ln_stats, rows, D, eps, s));
  if (p.block_fused()) {
    TableRef t;
    if (int rc = get_tables(N, &t, s)) return rc;
    const Ws w = ws_layout(p, B, N, D);
    DecimArgs a = decim_args(p, t, h, (char*)workspace, w, io != SMX_IO_F32 ? 2 : 4);
    a.in = x; a.out = y;
    filter_fwd(a, w_re, w_im, bias, 0, xk_save);
    a.ln_stats = (const cf*)ln_stats; a.ln_w = ln_w; a.ln_b = ln_b;
    set_drop(a, dc);
    if (int rc = pack_filter(a, p, w, workspace, workspace_bytes, w_re, w_im, D, F, nullptr, filter_pack,
                             s))
      return rc;
    HIP_TRY(launch_fused_block(a, p.nb, s, io));
    return SMX_OK;
  }
  // other plans: normalise into y, transform y in place (every kernel reads its whole input column
  // before the first store to it), add x
  float* hbuf = y;
  if (p.groups_only()) {    // no in-place form there: LayerNorm(x) goes to the workspace's row copy
    const Ws w = ws_layout(p, B, N, D);
    if (int rc = need_ws(workspace, workspace_bytes, w.total, "")) return rc;
    hbuf = (float*)((char*)workspace + w.rows);
  }
  HIP_TRY(launch_ln_apply(x, (const cf*)ln_stats, ln_w, ln_b, hbuf, rows, D, s));
  if (int rc = smx_forward_dropout(hbuf, w_re, w_im, bias, y, xk_save, workspace, workspace_bytes, B, N, D,
                                   F, 0, dropout_p, rng_state, filter_pack, stream))
    return rc;
  HIP_TRY(launch_add_rows(y, x, (size_t)rows * D, s));
  return SMX_OK;
}
int smx_block_forward_dropout(const float* x, const float* ln_w, const float* ln_b, float eps,
                              const float* w_re, const float* w_im, const float* bias, float* y,
                              float* xk_save, float* ln_stats, void* workspace,
                              size_t workspace_bytes, int B, int N, int D, int F, float dropout_p,
                              const void* rng_state, float* filter_pack, void* stream) {
  return block_forward_impl(x, ln_w, ln_b, eps, w_re, w_im, bias, y, xk_save, ln_stats, workspace, workspace_bytes, B, N,
                            D, F, dropout_p, rng_state, filter_pack, stream, SMX_IO_F32);
}
int smx_block_forward(const float* x, const float* ln_w, const float* ln_b, float eps,
                      const float* w_re, const float* w_im, const float* bias, float* y,
                      float* xk_save, float* ln_stats, void* workspace, size_t workspace_bytes,
                      int B, int N, int D, int F, void* stream) {
  return smx_block_forward_dropout(x, ln_w, ln_b, eps, w_re, w_im, bias, y, xk_save, ln_stats,
                                   workspace, workspace_bytes, B, N, D, F, 0.f, nullptr, nullptr,
                                   stream);
}

int smx_block_backward(const float* g, const float* x, const float* ln_stats, const float* ln_w,
                       const float* xk, const float* w_re, const float* w_im, float* grad_x,
                       float* g_ln_w, float* g_ln_b, float* gw_re, float* gw_im, float* gbias,
                       void* workspace, size_t workspace_bytes, int B, int N, int D, int F,
                       int phases, void* stream) {
  return smx_block_backward_dropout(g, x, ln_stats, ln_w, xk, w_re, w_im, grad_x, g_ln_w, g_ln_b, gw_re,
                                    gw_im, gbias, workspace, workspace_bytes, B, N, D, F, phases, 0.f,
                                    nullptr, nullptr, stream);
}

int smx_block_backward_dropout(const float* g, const float* x, const float* ln_stats,
                               const float* ln_w, const float* xk, const float* w_re,
                               const float* w_im, float* grad_x, float* g_ln_w, float* g_ln_b,
                               float* gw_re, float* gw_im, float* gbias, void* workspace,
                               size_t workspace_bytes, int B, int N, int D, int F, int phases,
                               float dropout_p, const void* rng_state, const float* filter_pack,
                               void* stream) {
  if (int rc = check_shape(B, N, D, F)) return rc;
  if (!ln_supported(D)) return fail(SMX_ERR_UNSUPPORTED, "LayerNorm width D=%d is not supported", D);
  if ((phases & 7) < 1 || phases > 15) return fail(SMX_ERR_INVALID, "phases must be a combination of 1, 2, 4");
  if ((phases & SMX_PHASE_INVERSE) && (!x || !ln_stats || !grad_x))
    return fail(SMX_ERR_INVALID, "x, ln_stats, grad_x must be non-NULL");
  if (g == grad_x || x == grad_x) return fail(SMX_ERR_INVALID, "grad_x must not alias g or x");
  if (D % 4 == 0 && (((uintptr_t)x | (uintptr_t)g | (uintptr_t)grad_x | (uintptr_t)ln_w) & 15))
    return fail(SMX_ERR_INVALID, "x, g, grad_x, ln_w must be 16-byte aligned");

  if (int rc = smx_backward_dropout(g, xk, w_re, w_im, grad_x, gw_re, gw_im, gbias, workspace,
                                    workspace_bytes, B, N, D, F, phases, dropout_p, rng_state,
                                    filter_pack, stream))
    return rc;
  if (phases & SMX_PHASE_INVERSE) {
    const Ws w = ws_layout(make_plan(layer_shape(B, N, D, F)), B, N, D);
    HIP_TRY(launch_ln_bwd(grad_x, x, g, (const cf*)ln_stats, ln_w, (float*)((char*)workspace + w.lnp),
                          g_ln_w, g_ln_b, (long long)B * N, D, (hipStream_t)stream));
  }
  return SMX_OK;
}

// ---- BicameralBlock's time path (smx_time.hip) ---------------------------------------------------------------------
static int dw_check(int B, int T, int C) {
  if (B <= 0 || T <= 0 || C <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: B=%d T=%d C=%d", B, T, C);
  if (B > 65535) return fail(SMX_ERR_UNSUPPORTED, "smx_dwconv3_* takes at most 65535 batch rows");
  if ((unsigned long long)B * ((T + 31) / 32) * ((C + 255) / 256) >= (1ull << 31))
    return fail(SMX_ERR_UNSUPPORTED, "smx_dwconv3_*: tensor too large for one launch");
  return SMX_OK;
}
// (the workspaces of the small ops lie behind the reserved header, as every layout: ws_layout)
static size_t dw_need(int B, int T, int C) { return WS_HEADER_BYTES + al(dwconv3_workspace_bytes(B, T, C)); }
int smx_dwconv3_workspace_bytes(int B, int T, int C, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  if (int rc = dw_check(B, T, C)) return rc;
  *out = dw_need(B, T, C);
  return SMX_OK;
}
int smx_dwconv3_forward(const float* x, const float* w, const float* bias, const float* scale, float* y, int B, int T,
                        int C, void* stream) {
  if (int rc = dw_check(B, T, C)) return rc;
  if (!x || !w || !y) return fail(SMX_ERR_INVALID, "x, w, y must be non-NULL");
  if (x == y) return fail(SMX_ERR_INVALID, "y must not alias x");
  HIP_TRY(launch_dwconv3_fwd(x, w, bias, scale, y, B, T, C, (hipStream_t)stream));
  return SMX_OK;
}
int smx_dwconv3_backward(const float* g, const float* x, const float* w, const float* bias, const float* scale,
                         float* grad_x, float* grad_w, float* grad_bias, float* grad_scale, void* workspace,
                         size_t workspace_bytes, int B, int T, int C, void* stream) {
  if (int rc = dw_check(B, T, C)) return rc;
  if (!g || !x || !w) return fail(SMX_ERR_INVALID, "g, x, w must be non-NULL");
  if (grad_x == g || grad_x == x) return fail(SMX_ERR_INVALID, "grad_x must not alias g or x");
  if (grad_scale && !scale) return fail(SMX_ERR_INVALID, "grad_scale without scale");
  if (int rc = need_ws(workspace, workspace_bytes, dw_need(B, T, C), "smx_dwconv3_workspace_bytes")) return rc;
  HIP_TRY(launch_dwconv3_bwd(g, x, w, bias, scale, grad_x, grad_w, grad_bias, grad_scale,
                             (float*)((char*)workspace + WS_HEADER_BYTES), B, T, C, (hipStream_t)stream));
  return SMX_OK;
}

// ---- SpectralLayerNorm (smx_time.hip) ---------------------------------------------------------------------------------
int smx_spectral_ln_supported(int C) { return spectral_ln_supported(C) ? 1 : 0; }
static int sln_check(int B, int F, int C) {
  if (B <= 0 || F <= 0 || C <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: B=%d F=%d C=%d", B, F, C);
  if (!spectral_ln_supported(C)) return fail(SMX_ERR_UNSUPPORTED, "smx_spectral_ln_* takes C <= 1024, got %d", C);
  if ((long long)B * F >= (1ll << 33)) return fail(SMX_ERR_UNSUPPORTED, "too many rows");
  return SMX_OK;
}
int smx_spectral_ln_forward(const float* z, const float* gamma, const float* beta, float eps, float* out, int planar,
                            int B, int F, int C, void* stream) {
  if (int rc = sln_check(B, F, C)) return rc;
  if (!z || !gamma || !beta || !out) return fail(SMX_ERR_INVALID, "z, gamma, beta, out must be non-NULL");
  if (((uintptr_t)z | (uintptr_t)out) & 7) return fail(SMX_ERR_INVALID, "z and out must be 8-byte aligned");
  HIP_TRY(launch_spectral_ln_fwd((const cf*)z, gamma, beta, eps, (cf*)out, planar, B, F, C, (hipStream_t)stream));
  return SMX_OK;
}
int smx_spectral_ln_backward(const float* g, const float* z, const float* gamma, const float* beta, float eps,
                             float* grad_z, float* grad_gamma, float* grad_beta, int planar, int B, int F, int C,
                             void* stream) {
  if (int rc = sln_check(B, F, C)) return rc;
  if (!g || !z || !gamma || !beta) return fail(SMX_ERR_INVALID, "g, z, gamma, beta must be non-NULL");
  if (((uintptr_t)g | (uintptr_t)z | (uintptr_t)grad_z) & 7) return fail(SMX_ERR_INVALID, "g, z, grad_z must be 8-byte aligned");
  HIP_TRY(launch_spectral_ln_bwd((const cf*)g, (const cf*)z, gamma, beta, eps, (cf*)grad_z, grad_gamma, grad_beta, planar,
                                 B, F, C, (hipStream_t)stream));
  return SMX_OK;
}
static int planar_check(int B, int F, int C) {
  if (B <= 0 || F <= 0 || C <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: B=%d F=%d C=%d", B, F, C);
  return SMX_OK;
}
int smx_planar_cmul_forward(const float* h, const float* f_re, const float* f_im, float* out, int B, int F, int C,
                            void* stream) {
  if (int rc = planar_check(B, F, C)) return rc;
  if (!h || !f_re || !f_im || !out) return fail(SMX_ERR_INVALID, "h, f_re, f_im, out must be non-NULL");
  HIP_TRY(launch_pcmul_fwd(h, f_re, f_im, out, B, F, C, (hipStream_t)stream));
  return SMX_OK;
}
int smx_planar_cmul_backward(const float* g, const float* h, const float* f_re, const float* f_im, float* grad_h,
                             float* grad_f_re, float* grad_f_im, int B, int F, int C, void* stream) {
  if (int rc = planar_check(B, F, C)) return rc;
  if (!g || !h || !f_re || !f_im) return fail(SMX_ERR_INVALID, "g, h, f_re, f_im must be non-NULL");
  HIP_TRY(launch_pcmul_bwd(g, h, f_re, f_im, grad_h, grad_f_re, grad_f_im, B, F, C, (hipStream_t)stream));
  return SMX_OK;
}
int smx_planar_add(const float* a, const float* planar, float* y, long long n, void* stream) {
  if (n <= 0 || !planar || !y) return fail(SMX_ERR_INVALID, "n must be positive, planar and y non-NULL");
  if (((uintptr_t)a | (uintptr_t)y) & 7) return fail(SMX_ERR_INVALID, "a and y must be 8-byte aligned");
  HIP_TRY(launch_add_planar((const cf*)a, planar, (cf*)y, n, (hipStream_t)stream));
  return SMX_OK;
}
int smx_planar_split(const float* g, float* planar, long long n, void* stream) {
  if (n <= 0 || !g || !planar) return fail(SMX_ERR_INVALID, "n must be positive, g and planar non-NULL");
  if ((uintptr_t)g & 7) return fail(SMX_ERR_INVALID, "g must be 8-byte aligned");
  HIP_TRY(launch_to_planar((const cf*)g, planar, n, (hipStream_t)stream));
  return SMX_OK;
}

// ---- the gate chain of the twin blocks (smx_time.hip) -------------------------------------------------------------------
static int gate_check(int B, int F, int C) {
  if (B <= 0 || F <= 0 || C <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: B=%d F=%d C=%d", B, F, C);
  if (C % 2) return fail(SMX_ERR_UNSUPPORTED, "smx_spectral_gate_* takes an even channel count, got %d", C);
  if (B > 65535) return fail(SMX_ERR_UNSUPPORTED, "smx_spectral_gate_* takes at most 65535 batch rows");
  return SMX_OK;
}
static size_t gate_need(int B, int F, int C) { return WS_HEADER_BYTES + al(gate_workspace_bytes(B, F, C)); }
int smx_spectral_gate_workspace_bytes(int B, int F, int C, size_t* out) {
  if (int rc = gate_check(B, F, C)) return rc;
  if (!out) return fail(SMX_ERR_INVALID, "out must be non-NULL");
  *out = gate_need(B, F, C);
  return SMX_OK;
}
int smx_spectral_gate_forward(const float* x, const float* a, const float* u, const float* p, const float* q,
                              const float* m, float* y, int B, int F, int C, void* stream) {
  if (int rc = gate_check(B, F, C)) return rc;
  if (!x || !a || !y) return fail(SMX_ERR_INVALID, "x, a, y must be non-NULL");
  if (((uintptr_t)x | (uintptr_t)y) & 15) return fail(SMX_ERR_INVALID, "x and y must be 16-byte aligned");
  if ((uintptr_t)a & 7) return fail(SMX_ERR_INVALID, "a must be 8-byte aligned");
  HIP_TRY(launch_gate_fwd((const cf*)x, (const cf*)a, u, p, q, m, (cf*)y, B, F, C, (hipStream_t)stream));
  return SMX_OK;
}
int smx_spectral_gate_backward(const float* g, const float* x, const float* a, const float* u, const float* p,
                               const float* q, const float* m, float* grad_x, float* s1, float* rc, float* rp,
                               void* workspace, size_t workspace_bytes, int B, int F, int C, void* stream) {
  if (int r = gate_check(B, F, C)) return r;
  if (!g || !x || !a) return fail(SMX_ERR_INVALID, "g, x, a must be non-NULL");
  if (((uintptr_t)g | (uintptr_t)x | (uintptr_t)grad_x) & 15) return fail(SMX_ERR_INVALID, "g, x, grad_x must be 16-byte aligned");
  if (((uintptr_t)a | (uintptr_t)s1) & 7) return fail(SMX_ERR_INVALID, "a and s1 must be 8-byte aligned");
  if (grad_x == g || grad_x == x) return fail(SMX_ERR_INVALID, "grad_x must not alias g or x");
  if (int r = need_ws(workspace, workspace_bytes, gate_need(B, F, C), "smx_spectral_gate_workspace_bytes")) return r;
  HIP_TRY(launch_gate_bwd((const cf*)g, (const cf*)x, (const cf*)a, u, p, q, m, (cf*)grad_x, (cf*)s1, rc, rp,
                          (cf*)((char*)workspace + WS_HEADER_BYTES), B, F, C, (hipStream_t)stream));
  return SMX_OK;
}

// ---- BicameralBlock's fusion line (smx_time.hip) --------------------------------------------------------------------------
static size_t mix_need() { return WS_HEADER_BYTES + al(mix_workspace_bytes()); }
int smx_mix_workspace_bytes(size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out must be non-NULL");
  *out = mix_need();
  return SMX_OK;
}
static int mix_check(long long n, const void* p0, const void* p1, const void* p2, const void* p3, const void* p4) {
  if (n <= 0 || n % 4) return fail(SMX_ERR_UNSUPPORTED, "smx_mix_* takes a positive element count that is a multiple of 4, got %lld", n);
  if (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3 | (uintptr_t)p4) & 15)
    return fail(SMX_ERR_INVALID, "tensors must be 16-byte aligned");
  return SMX_OK;
}
int smx_mix_forward(const float* r, const float* a, const float* b, const float* c, const float* w, float c3, float* out,
                    long long n, void* stream) {
  if (!r || !a || !b || !w || !out) return fail(SMX_ERR_INVALID, "r, a, b, w, out must be non-NULL");
  if (int rc = mix_check(n, r, a, b, c, out)) return rc;
  HIP_TRY(launch_mix_fwd(r, a, b, c, w, c3, out, n, (hipStream_t)stream));
  return SMX_OK;
}
int smx_mix_backward(const float* g, const float* a, const float* b, const float* w, float c3, float* grad_a, float* grad_b,
                     float* grad_c, float* grad_w, void* workspace, size_t workspace_bytes, long long n, void* stream) {
  if (!g || !a || !b || !w) return fail(SMX_ERR_INVALID, "g, a, b, w must be non-NULL");
  if (int rc = mix_check(n, g, a, b, grad_a, grad_b)) return rc;
  if ((uintptr_t)grad_c & 15) return fail(SMX_ERR_INVALID, "tensors must be 16-byte aligned");
  if (int rc = need_ws(workspace, workspace_bytes, mix_need(), "smx_mix_workspace_bytes")) return rc;
  HIP_TRY(launch_mix_bwd(g, a, b, w, c3, grad_a, grad_b, grad_c, grad_w, (float*)((char*)workspace + WS_HEADER_BYTES), n,
                         (hipStream_t)stream));
  return SMX_OK;
}


// ---- EnhancedSpectralBlock row lines (smx_enh.hip) ----
int smx_enh_supported(int D) { return enh_supported(D) ? 1 : 0; }
static size_t enh_need(int B, int T, int D) { return WS_HEADER_BYTES + al(enh_part_floats((long long)B * T, D) * sizeof(float)); }
int smx_enh_workspace_bytes(int B, int T, int D, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out must be non-NULL");
  if (B <= 0 || T <= 0 || D <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: B=%d T=%d D=%d", B, T, D);
  *out = enh_need(B, T, D);
  return SMX_OK;
}
static int enh_check(int B, int T, int D, std::initializer_list<const void*> ptrs) {
  if (B <= 0 || T <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: B=%d T=%d D=%d", B, T, D);
  if (!enh_supported(D)) return fail(SMX_ERR_UNSUPPORTED, "the enhanced-block row kernels take an even D <= %d, got %d", ENH_MAX_D, D);
  for (const void* p : ptrs)
    if ((uintptr_t)p & 15) return fail(SMX_ERR_INVALID, "tensors must be 16-byte aligned");
  return SMX_OK;
}
static int enh_ws(void* workspace, size_t workspace_bytes, int B, int T, int D, float** part) {
  if (int rc = need_ws(workspace, workspace_bytes, enh_need(B, T, D), "smx_enh_workspace_bytes")) return rc;
  *part = (float*)((char*)workspace + WS_HEADER_BYTES);
  return SMX_OK;
}
int smx_rope_norm_forward(const float* x, const float* rotation, int rot_rows, const float* ln1_w, const float* ln1_b,
                          const float* ln2_w, const float* ln2_b, float eps1, float eps2, float* x1, float* h2,
                          float* stats, int B, int T, int D, int norm, float dropout_p, const void* rng_state,
                          void* stream) {
  if (!x || !rotation || !x1) return fail(SMX_ERR_INVALID, "x, rotation, x1 must be non-NULL");
  if (norm && (!h2 || !stats)) return fail(SMX_ERR_INVALID, "h2 and stats must be non-NULL with norm != 0");
  if (int rc = enh_check(B, T, D, {x, rotation, ln1_w, ln1_b, ln2_w, ln2_b, x1, h2, stats})) return rc;
  if (T > rot_rows) return fail(SMX_ERR_INVALID, "T = %d is longer than the rotation table (%d rows)", T, rot_rows);
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  if (!norm && dc.thr) return fail(SMX_ERR_INVALID, "dropout needs norm != 0 (the block line)");
  HIP_TRY(launch_rope_fwd(x, rotation, ln1_w, ln1_b, ln2_w, ln2_b, eps1, eps2, x1, h2, (cf*)stats, B, T, D, norm != 0,
                          dc.thr, dc.scale, dc.rng, (hipStream_t)stream));
  return SMX_OK;
}
int smx_rope_norm_backward(const float* g1, const float* gh2, const float* x, const float* rotation, int rot_rows,
                           const float* ln1_w, const float* ln1_b, const float* ln2_w, const float* stats, float* grad_x,
                           float* g_ln1_w, float* g_ln1_b, float* g_ln2_w, float* g_ln2_b, void* workspace,
                           size_t workspace_bytes, int B, int T, int D, int norm, float dropout_p,
                           const void* rng_state, void* stream) {
  if (!g1 || !rotation || !grad_x) return fail(SMX_ERR_INVALID, "g1, rotation, grad_x must be non-NULL");
  if (norm && (!gh2 || !x || !stats)) return fail(SMX_ERR_INVALID, "gh2, x and stats must be non-NULL with norm != 0");
  if (int rc = enh_check(B, T, D, {g1, gh2, x, rotation, ln1_w, ln1_b, ln2_w, stats, grad_x})) return rc;
  if (T > rot_rows) return fail(SMX_ERR_INVALID, "T = %d is longer than the rotation table (%d rows)", T, rot_rows);
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  if (!norm && dc.thr) return fail(SMX_ERR_INVALID, "dropout needs norm != 0 (the block line)");
  float* part = nullptr;
  if (norm)
    if (int rc = enh_ws(workspace, workspace_bytes, B, T, D, &part)) return rc;
  HIP_TRY(launch_rope_bwd(g1, gh2, x, rotation, ln1_w, ln1_b, ln2_w, (const cf*)stats, grad_x, g_ln1_w, g_ln1_b, g_ln2_w,
                          g_ln2_b, part, B, T, D, norm != 0, dc.thr, dc.scale, dc.rng, (hipStream_t)stream));
  return SMX_OK;
}
int smx_residual_norm_forward(const float* x1, const float* p, const float* ln_w, const float* ln_b, float eps,
                              float* x2, float* h3, float* stats, int B, int T, int D, float dropout_p,
                              const void* rng_state, void* stream) {
  if (!x1 || !p || !x2 || !h3 || !stats) return fail(SMX_ERR_INVALID, "x1, p, x2, h3, stats must be non-NULL");
  if (int rc = enh_check(B, T, D, {x1, p, ln_w, ln_b, x2, h3, stats})) return rc;
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  HIP_TRY(launch_res_fwd(x1, p, ln_w, ln_b, eps, x2, h3, (cf*)stats, B, T, D, dc.thr, dc.scale, dc.rng,
                         (hipStream_t)stream));
  return SMX_OK;
}
int smx_residual_norm_backward(const float* g2, const float* gh3, const float* x2, const float* ln_w, const float* stats,
                               float* grad_x1, float* grad_p, float* g_ln_w, float* g_ln_b, void* workspace,
                               size_t workspace_bytes, int B, int T, int D, float dropout_p, const void* rng_state,
                               void* stream) {
  if (!g2 || !gh3 || !x2 || !stats || !grad_x1) return fail(SMX_ERR_INVALID, "g2, gh3, x2, stats, grad_x1 must be non-NULL");
  if (int rc = enh_check(B, T, D, {g2, gh3, x2, ln_w, stats, grad_x1, grad_p})) return rc;
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  if (dc.thr && !grad_p) return fail(SMX_ERR_INVALID, "grad_p must be non-NULL with dropout p > 0");
  float* part = nullptr;
  if (int rc = enh_ws(workspace, workspace_bytes, B, T, D, &part)) return rc;
  HIP_TRY(launch_res_bwd(g2, gh3, x2, ln_w, (const cf*)stats, grad_x1, grad_p, g_ln_w, g_ln_b, part, B, T, D, dc.thr,
                         dc.scale, dc.rng, (hipStream_t)stream));
  return SMX_OK;
}
int smx_gate_blend_forward(const float* a, const float* v, const float* x2, const float* ln_w, const float* ln_b,
                           float eps, float* x3, float* stats, int B, int T, int D, float dropout_p,
                           const void* rng_state, void* stream) {
  if (!a || !v || !x3 || !stats) return fail(SMX_ERR_INVALID, "a, v, x3, stats must be non-NULL");
  if (int rc = enh_check(B, T, D, {a, v, x2, ln_w, ln_b, x3, stats})) return rc;
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  HIP_TRY(launch_gate_blend_fwd(a, v, x2, ln_w, ln_b, eps, x3, (cf*)stats, B, T, D, dc.thr, dc.scale, dc.rng,
                                (hipStream_t)stream));
  return SMX_OK;
}
int smx_gate_blend_backward(const float* g3, const float* a, const float* v, const float* ln_w, const float* ln_b,
                            const float* stats, float* grad_a, float* grad_v, float* g_ln_w, float* g_ln_b,
                            void* workspace, size_t workspace_bytes, int B, int T, int D, float dropout_p,
                            const void* rng_state, void* stream) {
  if (!g3 || !a || !v || !stats || !grad_a || !grad_v)
    return fail(SMX_ERR_INVALID, "g3, a, v, stats, grad_a, grad_v must be non-NULL");
  if (int rc = enh_check(B, T, D, {g3, a, v, ln_w, ln_b, stats, grad_a, grad_v})) return rc;
  DropCfg dc;
  if (int rc = drop_cfg(dropout_p, rng_state, &dc)) return rc;
  float* part = nullptr;
  if (int rc = enh_ws(workspace, workspace_bytes, B, T, D, &part)) return rc;
  HIP_TRY(launch_gate_blend_bwd(g3, a, v, ln_w, ln_b, (const cf*)stats, grad_a, grad_v, g_ln_w, g_ln_b, part, B, T, D,
                                dc.thr, dc.scale, dc.rng, (hipStream_t)stream));
  return SMX_OK;
}

// ---- 2-byte activations (bf16 / fp16 x, y, g, grad_x) ---------------------------------------------------------------
// Replaces: reference fft_tensor/spectral_layers.py:88 (fft), :94-109 (filter), :112-116 (ifft, bias) and their autograd
// backward for half-precision activations (the reference's torch.fft refuses bf16 and takes fp16 for powers of two only).
// Same implementation (forward_impl / backward_impl), plan, launches, work items and summation order as the f32
// entries; only the streaming kernels' row I/O differs (the IO instances of k_fused / k_split_a / k_split_b), so the
// outputs are the f32 outputs rounded once (include/smx.h).
int smx_io_supported(int B, int N, int D, int F, int io) {
  if (io_check(io) || check_shape(B, N, D, F)) return 0;
  if (io == SMX_IO_F32) return 1;
  return make_plan(layer_shape(B, N, D, F)).io_native() ? 1 : 0;
}

int smx_forward_io(const void* x, const float* w_re, const float* w_im, const float* bias, void* y,
                   float* xk_save, void* workspace, size_t workspace_bytes, int B, int N, int D, int F,
                   int conj_w, float dropout_p, const void* rng_state, float* filter_pack, void* stream, int io) {
  if (int rc = io_check(io)) return rc;
  if (int rc = check_shape(B, N, D, F)) return rc;
  return forward_impl(layer_shape(B, N, D, F), (const float*)x, w_re, w_im, bias, (float*)y, xk_save, workspace,
                      workspace_bytes, conj_w, dropout_p, rng_state, filter_pack, stream, nullptr, io);
}

int smx_backward_io(const void* g, const float* xk, const float* w_re, const float* w_im, void* grad_x,
                    float* gw_re, float* gw_im, float* gbias, void* workspace, size_t workspace_bytes, int B,
                    int N, int D, int F, int phases, float dropout_p, const void* rng_state,
                    const float* filter_pack, void* stream, int io) {
  if (int rc = io_check(io)) return rc;
  if (int rc = check_shape(B, N, D, F)) return rc;
  return backward_impl(layer_shape(B, N, D, F), (const float*)g, xk, w_re, w_im, (float*)grad_x, gw_re, gw_im, gbias,
                       workspace, workspace_bytes, phases, dropout_p, rng_state, filter_pack, stream, nullptr, nullptr,
                       io, -1);
}

// ---- 2-byte activations of the convolution (bf16 / fp16 x, y, g, grad_x) -------------------------------------------
// Replaces: reference fft_lm/train_fixed_full.py:515-555 and its autograd backward for half-precision activations.
// Same implementation (conv_forward_impl / conv_backward_impl), plan, launch, work items and summation order as
// smx_conv_forward / smx_conv_backward; only k_conv1's row I/O differs (its IO instances), so the outputs are the
// f32 outputs rounded once (include/smx.h).
int smx_conv_io_supported(const smx_shape* shape, int io) {
  Shape h; Plan p;
  if (io_check(io) || conv_shape(shape, &h) || !conv_plan(h, &p)) return 0;
  return io == SMX_IO_F32 || p.conv1 ? 1 : 0;
}

int smx_conv_forward_io(const smx_shape* shape, const void* x, const float* h_re, const float* h_im,
                        const float* row_scale, void* y, float* x_spectra, void* workspace,
                        size_t workspace_bytes, int io, void* stream) {
  if (int rc = io_check(io)) return rc;
  return conv_forward_impl(shape, (const float*)x, h_re, h_im, row_scale, (float*)y, x_spectra, workspace,
                           workspace_bytes, io, stream);
}

int smx_conv_backward_io(const smx_shape* shape, const void* g, const float* x_spectra, const float* h_re,
                         const float* h_im, const float* row_scale, void* grad_x, float* grad_h_re,
                         float* grad_h_im, float* grad_row_scale, void* workspace, size_t workspace_bytes,
                         int io, void* stream) {
  if (int rc = io_check(io)) return rc;
  return conv_backward_impl(shape, (const float*)g, x_spectra, h_re, h_im, row_scale, (float*)grad_x, grad_h_re,
                            grad_h_im, grad_row_scale, workspace, workspace_bytes, io, stream);
}

// ---- 2-byte activations of the fused block line (bf16 / fp16 x, y, g, grad_x) -----------------------------------------
// Replaces: reference fft_tensor/spectral_layers.py:185 (x + spectral_mix(norm1(x)), with :154-158, :162) and its autograd
// backward for half-precision activations -- there three torch ops with three roundings of the activation.  Same plan,
// launches, work items and summation order as smx_block_forward_dropout / smx_block_backward_dropout; only the row I/O
// of k_ln_stats, k_fused_blk, k_fused (mode 1: 2-byte g in, f32 grad_h out) and k_ln_bwd differs.
int smx_block_io_supported(int B, int N, int D, int F, int io) {
  if (io_check(io) || check_shape(B, N, D, F)) return 0;
  if (io == SMX_IO_F32) return smx_block_supported(D);
  return block_io_native(make_plan(layer_shape(B, N, D, F)), D) ? 1 : 0;
}

int smx_block_forward_io(const void* x, const float* ln_w, const float* ln_b, float eps, const float* w_re,
                         const float* w_im, const float* bias, void* y, float* xk_save, float* ln_stats,
                         void* workspace, size_t workspace_bytes, int B, int N, int D, int F, float dropout_p,
                         const void* rng_state, float* filter_pack, void* stream, int io) {
  if (int rc = io_check(io)) return rc;
  return block_forward_impl((const float*)x, ln_w, ln_b, eps, w_re, w_im, bias, (float*)y, xk_save, ln_stats, workspace,
                            workspace_bytes, B, N, D, F, dropout_p, rng_state, filter_pack, stream, io);
}

int smx_block_backward_io(const void* g, const void* x, const float* ln_stats, const float* ln_w, const float* xk,
                          const float* w_re, const float* w_im, void* grad_x, float* g_ln_w, float* g_ln_b,
                          float* gw_re, float* gw_im, float* gbias, float* grad_h, void* workspace,
                          size_t workspace_bytes, int B, int N, int D, int F, int phases, float dropout_p,
                          const void* rng_state, const float* filter_pack, void* stream, int io) {
  if (int rc = io_check(io)) return rc;
  if (io == SMX_IO_F32)
    return smx_block_backward_dropout((const float*)g, (const float*)x, ln_stats, ln_w, xk, w_re, w_im, (float*)grad_x,
                                      g_ln_w, g_ln_b, gw_re, gw_im, gbias, workspace, workspace_bytes, B, N, D, F,
                                      phases, dropout_p, rng_state, filter_pack, stream);
  if (int rc = check_shape(B, N, D, F)) return rc;
  if (!ln_supported(D)) return fail(SMX_ERR_UNSUPPORTED, "LayerNorm width D=%d is not supported", D);
  if ((phases & 7) < 1 || phases > 15) return fail(SMX_ERR_INVALID, "phases must be a combination of 1, 2, 4");
  const Shape h = layer_shape(B, N, D, F);
  if (!block_io_native(make_plan(h), D)) return fail(SMX_ERR_UNSUPPORTED, BLOCK_IO_PLANS);
  if (!grad_h || ((uintptr_t)grad_h & 15))
    return fail(SMX_ERR_INVALID, "grad_h, a (B, N, D) f32 scratch, must be non-NULL and 16-byte aligned");
  if ((phases & SMX_PHASE_INVERSE) && (!x || !ln_stats || !grad_x))
    return fail(SMX_ERR_INVALID, "x, ln_stats, grad_x must be non-NULL");
  if (g == grad_x || x == grad_x) return fail(SMX_ERR_INVALID, "grad_x must not alias g or x");
  if (((uintptr_t)x | (uintptr_t)g | (uintptr_t)grad_x) & 7)
    return fail(SMX_ERR_INVALID, "2-byte x, g, grad_x (D %% 4 == 0) must be 8-byte aligned");
  if ((uintptr_t)ln_w & 15) return fail(SMX_ERR_INVALID, "ln_w must be 16-byte aligned");

  if (int rc = backward_impl(h, (const float*)g, xk, w_re, w_im, grad_h, gw_re, gw_im, gbias, workspace, workspace_bytes,
                             phases, dropout_p, rng_state, filter_pack, stream, nullptr, nullptr, io, SMX_IO_F32))
    return rc;
  if (phases & SMX_PHASE_INVERSE) {
    const Ws w = ws_layout(make_plan(h), B, N, D);
    HIP_TRY(launch_ln_bwd_io(grad_h, x, g, grad_x, (const cf*)ln_stats, ln_w, (float*)((char*)workspace + w.lnp), g_ln_w,
                             g_ln_b, (long long)B * N, D, (hipStream_t)stream, io));
  }
  return SMX_OK;
}

// ---- SpectralEMA scan (smx_ema.hip) ---------------------------------------------------------------------------------------
static int ema_check(int mode, int B, int S, int F) {
  if (mode != SMX_EMA_ALIGNED && mode != SMX_EMA_POLAR)
    return fail(SMX_ERR_INVALID, "mode must be SMX_EMA_ALIGNED (0) or SMX_EMA_POLAR (1), got %d", mode);
  if (B <= 0 || F <= 0) return fail(SMX_ERR_INVALID, "B and F must be positive: B=%d F=%d", B, F);
  if (S < 0) return fail(SMX_ERR_INVALID, "the chunk count must not be negative, got %d", S);
  if ((long long)B * F >= (1ll << 31)) return fail(SMX_ERR_UNSUPPORTED, "smx_ema_*: more than 2^31 chains");
  return SMX_OK;
}
static int ema_tokens_src(const void* tokens, int token_bytes, long long row_stride, int B, int T, int L, EmaSrc* src) {
  if (L < 2 || L > 64) return fail(SMX_ERR_INVALID, "chunk length L must be in 2..64, got %d", L);
  if (T < 0) return fail(SMX_ERR_INVALID, "T must not be negative, got %d", T);
  const int S = T / L;
  int kind;
  if (int rc = token_src(tokens, token_bytes, row_stride, T, S > 0, &kind)) return rc;
  *src = EmaSrc{tokens, kind, row_stride, B, S, L / 2 + 1, L};
  return SMX_OK;
}
static size_t ema_need(int B, int S, int F) { return WS_HEADER_BYTES + al(ema_states_bytes(B, S, F)) + al(ema_part_bytes(B, F)); }
static int ema_fwd(const EmaSrc& src, int mode, const float* init, const float* rho_logit, const float* theta_raw,
                   float* out, void* stream) {
  if (!rho_logit || !out || (mode == SMX_EMA_ALIGNED && !theta_raw))
    return fail(SMX_ERR_INVALID, "rho_logit, theta_raw (aligned mode), out must be non-NULL");
  if (((uintptr_t)init | (uintptr_t)out) & 7) return fail(SMX_ERR_INVALID, "init and out must be 8-byte aligned");
  HIP_TRY(launch_ema(src, mode == SMX_EMA_POLAR, (const cf*)init, rho_logit, theta_raw, (cf*)out, (hipStream_t)stream));
  return SMX_OK;
}
static int ema_bwd(const EmaSrc& src, int mode, const float* g, const float* init, const float* rho_logit,
                   const float* theta_raw, float* grad_chunks, float* grad_init, float* grad_rho_logit,
                   float* grad_theta_raw, void* workspace, size_t workspace_bytes, void* stream) {
  if (!g || !rho_logit || (mode == SMX_EMA_ALIGNED && !theta_raw))
    return fail(SMX_ERR_INVALID, "g, rho_logit, theta_raw (aligned mode) must be non-NULL");
  if (((uintptr_t)g | (uintptr_t)init | (uintptr_t)grad_chunks | (uintptr_t)grad_init) & 7)
    return fail(SMX_ERR_INVALID, "g, init, grad_chunks, grad_init must be 8-byte aligned");
  if (grad_chunks && grad_chunks == src.ptr) return fail(SMX_ERR_INVALID, "grad_chunks must not alias chunks");
  if (int rc = need_ws(workspace, workspace_bytes, ema_need(src.B, src.S, src.F), "smx_ema_workspace_bytes")) return rc;
  char* states = (char*)workspace + WS_HEADER_BYTES;
  HIP_TRY(launch_ema_bwd(src, mode == SMX_EMA_POLAR, (const cf*)g, (const cf*)init, rho_logit, theta_raw, (cf*)grad_chunks,
                         (cf*)grad_init, grad_rho_logit, grad_theta_raw, (cf*)states,
                         (float*)(states + al(ema_states_bytes(src.B, src.S, src.F))), (hipStream_t)stream));
  return SMX_OK;
}
int smx_ema_workspace_bytes(int B, int S, int F, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out must be non-NULL");
  if (int rc = ema_check(SMX_EMA_ALIGNED, B, S, F)) return rc;
  *out = ema_need(B, S, F);
  return SMX_OK;
}
int smx_ema_scan_forward(const float* chunks, const float* init, const float* rho_logit, const float* theta_raw,
                         float* out, int mode, int B, int S, int F, void* stream) {
  if (int rc = ema_check(mode, B, S, F)) return rc;
  if ((S > 0 && !chunks) || ((uintptr_t)chunks & 7))
    return fail(SMX_ERR_INVALID, "chunks must be non-NULL and 8-byte aligned");
  return ema_fwd(EmaSrc{chunks, 0, 0, B, S, F, 0}, mode, init, rho_logit, theta_raw, out, stream);
}
int smx_ema_scan_backward(const float* g, const float* chunks, const float* init, const float* rho_logit,
                          const float* theta_raw, float* grad_chunks, float* grad_init, float* grad_rho_logit,
                          float* grad_theta_raw, void* workspace, size_t workspace_bytes, int mode, int B, int S, int F,
                          void* stream) {
  if (int rc = ema_check(mode, B, S, F)) return rc;
  if ((S > 0 && !chunks) || ((uintptr_t)chunks & 7))
    return fail(SMX_ERR_INVALID, "chunks must be non-NULL and 8-byte aligned");
  return ema_bwd(EmaSrc{chunks, 0, 0, B, S, F, 0}, mode, g, init, rho_logit, theta_raw, grad_chunks, grad_init,
                 grad_rho_logit, grad_theta_raw, workspace, workspace_bytes, stream);
}
int smx_ema_tokens_forward(const void* tokens, int token_bytes, long long row_stride, const float* init,
                           const float* rho_logit, const float* theta_raw, float* out, int mode, int B, int T, int L,
                           void* stream) {
  EmaSrc src;
  if (int rc = ema_tokens_src(tokens, token_bytes, row_stride, B, T, L, &src)) return rc;
  if (int rc = ema_check(mode, B, src.S, src.F)) return rc;
  return ema_fwd(src, mode, init, rho_logit, theta_raw, out, stream);
}
int smx_ema_tokens_backward(const float* g, const void* tokens, int token_bytes, long long row_stride, const float* init,
                            const float* rho_logit, const float* theta_raw, float* grad_init, float* grad_rho_logit,
                            float* grad_theta_raw, void* workspace, size_t workspace_bytes, int mode, int B, int T, int L,
                            void* stream) {
  EmaSrc src;
  if (int rc = ema_tokens_src(tokens, token_bytes, row_stride, B, T, L, &src)) return rc;
  if (int rc = ema_check(mode, B, src.S, src.F)) return rc;
  return ema_bwd(src, mode, g, init, rho_logit, theta_raw, nullptr, grad_init, grad_rho_logit, grad_theta_raw, workspace,
                 workspace_bytes, stream);
}

// ---- word-structure heads: targets (smx_ema.hip) and the O-neuron row head (smx_block.hip) ----------------------------------
int smx_word_targets(const void* tokens, int token_bytes, long long row_stride, float* phase, float* boundary, int B,
                     int T, void* stream) {
  if (B <= 0 || T <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: B=%d T=%d", B, T);
  if (T > WT_MAX_T) return fail(SMX_ERR_INVALID, "T must be at most %d, got %d", WT_MAX_T, T);
  if ((long long)B * T >= (1ll << 31)) return fail(SMX_ERR_INVALID, "B*T too large");
  int kind;
  if (int rc = token_src(tokens, token_bytes, row_stride, T, true, &kind)) return rc;
  if (!phase && !boundary) return fail(SMX_ERR_INVALID, "phase and boundary are both NULL");
  if (((uintptr_t)phase & 7) || ((uintptr_t)boundary & 3))
    return fail(SMX_ERR_INVALID, "phase must be 8-byte aligned and boundary 4-byte aligned");
  HIP_TRY(launch_word_targets(tokens, kind, row_stride, phase, boundary, B, T, (hipStream_t)stream));
  return SMX_OK;
}

static int head_check(long long R, int C, int O) {
  if (R <= 0 || C <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: R=%lld C=%d", R, C);
  if (O != 1 && O != 2) return fail(SMX_ERR_UNSUPPORTED, "the row head has O = 1 or 2 outputs, got %d", O);
  if (!ln_supported(C)) return fail(SMX_ERR_UNSUPPORTED, "LayerNorm width D=%d is not supported", C);
  if (R * C >= (1ll << 40)) return fail(SMX_ERR_INVALID, "R*C too large");
  return SMX_OK;
}
static size_t head_need(long long R, int C) { return WS_HEADER_BYTES + al(head_part_w_bytes(R, C)) + al(head_part_b_bytes(R)); }
int smx_head_supported(int C, int O) { return (O == 1 || O == 2) && ln_supported(C) ? 1 : 0; }
int smx_head_workspace_bytes(long long R, int C, int O, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out must be non-NULL");
  if (int rc = head_check(R, C, O)) return rc;
  *out = head_need(R, C);
  return SMX_OK;
}
int smx_head_forward(const float* h, const float* w, const float* b, float* y, long long R, int C, int O, void* stream) {
  if (int rc = head_check(R, C, O)) return rc;
  if (!h || !w || !y) return fail(SMX_ERR_INVALID, "h, w, y must be non-NULL");
  if (((uintptr_t)h | (uintptr_t)w) & 15) return fail(SMX_ERR_INVALID, "h and w must be 16-byte aligned");
  if (((uintptr_t)b | (uintptr_t)y) & 3) return fail(SMX_ERR_INVALID, "b and y must be 4-byte aligned");
  HIP_TRY(launch_head_fwd(h, w, b, y, R, C, O, (hipStream_t)stream));
  return SMX_OK;
}
int smx_head_backward(const float* g, const float* h, const float* w, float* grad_h, float* grad_w, float* grad_b,
                      void* workspace, size_t workspace_bytes, long long R, int C, int O, void* stream) {
  if (int rc = head_check(R, C, O)) return rc;
  if (!g || (grad_w && !h) || (grad_h && !w))
    return fail(SMX_ERR_INVALID, "g, h (with grad_w), w (with grad_h) must be non-NULL");
  if (((uintptr_t)h | (uintptr_t)w | (uintptr_t)grad_h) & 15)
    return fail(SMX_ERR_INVALID, "h, w and grad_h must be 16-byte aligned");
  if (((uintptr_t)g | (uintptr_t)grad_w | (uintptr_t)grad_b) & 3)
    return fail(SMX_ERR_INVALID, "g, grad_w and grad_b must be 4-byte aligned");
  if (grad_h && (grad_h == h || grad_h == g)) return fail(SMX_ERR_INVALID, "grad_h must not alias h or g");
  if (int rc = need_ws(workspace, workspace_bytes, head_need(R, C), "smx_head_workspace_bytes")) return rc;
  char* part_w = (char*)workspace + WS_HEADER_BYTES;
  HIP_TRY(launch_head_bwd(g, h, w, grad_h, grad_w, grad_b, (float*)part_w, (float*)(part_w + al(head_part_w_bytes(R, C))),
                          R, C, O, (hipStream_t)stream));
  return SMX_OK;
}

// ---- softmax cross-entropy (smx_block.hip) -----------------------------------------------------------------------------------
static int xent_check(long long R, int V) {
  if (R <= 0 || V <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: R=%lld V=%d", R, V);
  if (R >= (1ll << 31)) return fail(SMX_ERR_INVALID, "R too large");
  return SMX_OK;
}
static int xent_check_args(const char* fn, long long R, int V, long long row_stride, int reduction) {
  if (int rc = xent_check(R, V)) return rc;
  if (row_stride < V) return fail(SMX_ERR_INVALID, "%s: row_stride must be at least V", fn);
  if (reduction != SMX_XENT_MEAN && reduction != SMX_XENT_SUM && reduction != SMX_XENT_NONE)
    return fail(SMX_ERR_INVALID, "%s: reduction must be SMX_XENT_MEAN, _SUM or _NONE, got %d", fn, reduction);
  return SMX_OK;
}
static size_t xent_need(long long R) { return WS_HEADER_BYTES + al((size_t)xent_num_blocks(R) * 2 * sizeof(float)); }
int smx_xent_supported(int V) { return V >= 1 ? 1 : 0; }
int smx_xent_workspace_bytes(long long R, int V, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out must be non-NULL");
  if (int rc = xent_check(R, V)) return rc;
  *out = xent_need(R);
  return SMX_OK;
}
int smx_xent_forward(const float* logits, long long row_stride, const long long* targets, long long ignore_index,
                     int reduction, float* loss, float* lse, float* count, void* workspace, size_t workspace_bytes,
                     long long R, int V, void* stream) {
  if (int rc = xent_check_args("smx_xent_forward", R, V, row_stride, reduction)) return rc;
  if (!logits || !targets || !loss || !lse || !count)
    return fail(SMX_ERR_INVALID, "logits, targets, loss, lse, count must be non-NULL");
  if ((((uintptr_t)logits | (uintptr_t)loss | (uintptr_t)lse | (uintptr_t)count) & 3) || ((uintptr_t)targets & 7))
    return fail(SMX_ERR_INVALID, "logits, loss, lse, count must be 4-byte aligned and targets 8-byte aligned");
  if (int rc = need_ws(workspace, workspace_bytes, xent_need(R), "smx_xent_workspace_bytes")) return rc;
  HIP_TRY(launch_xent_fwd(logits, row_stride, targets, ignore_index, reduction, loss, lse, count,
                          (float*)((char*)workspace + WS_HEADER_BYTES), R, V, (hipStream_t)stream));
  return SMX_OK;
}
int smx_xent_backward(const float* g, const float* logits, long long row_stride, const long long* targets,
                      long long ignore_index, int reduction, const float* lse, const float* count, float* grad,
                      long long R, int V, void* stream) {
  if (int rc = xent_check_args("smx_xent_backward", R, V, row_stride, reduction)) return rc;
  if (!g || !logits || !targets || !lse || !count || !grad)
    return fail(SMX_ERR_INVALID, "g, logits, targets, lse, count, grad must be non-NULL");
  if ((((uintptr_t)g | (uintptr_t)logits | (uintptr_t)lse | (uintptr_t)count | (uintptr_t)grad) & 3) ||
      ((uintptr_t)targets & 7))
    return fail(SMX_ERR_INVALID, "g, logits, lse, count, grad must be 4-byte aligned and targets 8-byte aligned");
  if (grad == logits) return fail(SMX_ERR_INVALID, "grad must not alias logits");
  HIP_TRY(launch_xent_bwd(g, logits, row_stride, targets, ignore_index, reduction, lse, count, grad, R, V,
                          (hipStream_t)stream));
  return SMX_OK;
}

// ---- overlap-save chunk generation (smx_stream.hip) -----------------------------------------------------------------------
static int stream_check(const char* fn, int Bt, int T, int K, int C, int chunk, std::initializer_list<const void*> ptrs) {
  if (Bt < 1 || Bt > (1 << 24)) return fail(SMX_ERR_INVALID, "%s: Bt must be in 1..2^24, got %d", fn, Bt);
  if (!stream_supported(T, K, C, chunk))
    return fail(SMX_ERR_INVALID,
                "%s: unsupported shape T=%d K=%d C=%d chunk=%d (smx_stream_supported: a LayerNorm row width, "
                "1 <= chunk <= %d, 1 <= K <= %d, K - 1 + chunk <= T)", fn, T, K, C, chunk, STREAM_MAX_CHUNK, STREAM_MAX_K);
  for (const void* p : ptrs)
    if ((uintptr_t)p & 15) return fail(SMX_ERR_INVALID, "%s: tensors must be 16-byte aligned", fn);
  return SMX_OK;
}
int smx_stream_supported(int T, int K, int C, int chunk) { return stream_supported(T, K, C, chunk) ? 1 : 0; }
int smx_stream_push(const float* h, const float* ln_w, const float* ln_b, float eps, float* ring, float* sum, int* pos,
                    float* pooled, int Bt, int T, int C, int chunk, void* stream) {
  if (!h || !ring || !sum || !pos || !pooled)
    return fail(SMX_ERR_INVALID, "smx_stream_push: h, ring, sum, pos, pooled must be non-NULL");
  if ((uintptr_t)pos & 3) return fail(SMX_ERR_INVALID, "smx_stream_push: pos must be 4-byte aligned");
  if (int rc = stream_check("smx_stream_push", Bt, T, 1, C, chunk, {h, ln_w, ln_b, ring, sum, pooled})) return rc;
  HIP_TRY(launch_stream_push(h, ln_w, ln_b, eps, ring, sum, pos, pooled, Bt, T, C, chunk, (hipStream_t)stream));
  return SMX_OK;
}
int smx_stream_conv(const float* h, const float* ring, const int* pos, const float* taps, const float* scale,
                    const float* ln_w, const float* ln_b, float eps, float* h_out, float* ff_in, int Bt, int T, int K,
                    int C, int chunk, void* stream) {
  if (!h || !ring || !pos || !taps || !scale || !h_out)
    return fail(SMX_ERR_INVALID, "smx_stream_conv: h, ring, pos, taps, scale, h_out must be non-NULL");
  if (((uintptr_t)pos | (uintptr_t)taps) & 3)
    return fail(SMX_ERR_INVALID, "smx_stream_conv: pos and taps must be 4-byte aligned");
  if (int rc = stream_check("smx_stream_conv", Bt, T, K, C, chunk, {h, ring, scale, ln_w, ln_b, h_out, ff_in})) return rc;
  HIP_TRY(launch_stream_conv(h, ring, pos, taps, scale, ln_w, ln_b, eps, h_out, ff_in, Bt, T, K, C, chunk,
                             (hipStream_t)stream));
  return SMX_OK;
}

// ---- the byte sampler (smx_stream.hip) -------------------------------------------------------------------------------------
int smx_sample_supported(int V) { return V == SAMPLE_V ? 1 : 0; }
int smx_sample_bytes(const float* logits, long long row_stride, const void* recent, int token_bytes, int n_recent,
                     float temperature, float top_p, int top_k, float repetition_penalty, float presence_penalty,
                     float frequency_penalty, int ascii_only, int ban_cr, int max_run_length, const float* u,
                     long long* ids, float* probs, long long R, int V, void* stream) {
  if (R <= 0 || V <= 0) return fail(SMX_ERR_INVALID, "shape must be positive: R=%lld V=%d", R, V);
  if (V != SAMPLE_V) return fail(SMX_ERR_UNSUPPORTED, "the sampler draws bytes: V must be %d, got %d", SAMPLE_V, V);
  if (R >= (1ll << 31)) return fail(SMX_ERR_INVALID, "R too large");
  if (!logits || !u || !ids) return fail(SMX_ERR_INVALID, "logits, u, ids must be non-NULL");
  if (row_stride < V) return fail(SMX_ERR_INVALID, "row_stride must be at least V");
  int kind;                              // (the window's own NULL and alignment refusals follow: they read differently)
  if (int rc = token_src(nullptr, token_bytes, 0, 0, false, &kind)) return rc;
  if (n_recent < 0 || n_recent > SAMPLE_MAX_RECENT)
    return fail(SMX_ERR_INVALID, "n_recent must be in [0, %d], got %d", SAMPLE_MAX_RECENT, n_recent);
  if (n_recent > 0 && !recent) return fail(SMX_ERR_INVALID, "recent must be non-NULL with n_recent > 0");
  if (token_bytes == 8 && ((uintptr_t)recent & 7)) return fail(SMX_ERR_INVALID, "int64 recent ids must be 8-byte aligned");
  if ((((uintptr_t)logits | (uintptr_t)u | (uintptr_t)probs) & 3) || ((uintptr_t)ids & 7))
    return fail(SMX_ERR_INVALID, "logits, u, probs must be 4-byte aligned and ids 8-byte aligned");
  if (!(temperature > 0.f) || !std::isfinite(temperature))
    return fail(SMX_ERR_INVALID, "temperature must be positive and finite, got %g", (double)temperature);
  if (!(repetition_penalty > 0.f) || !std::isfinite(repetition_penalty))
    return fail(SMX_ERR_INVALID, "repetition_penalty must be positive and finite, got %g", (double)repetition_penalty);
  if (std::isnan(top_p)) return fail(SMX_ERR_INVALID, "top_p is NaN");
  if (!std::isfinite(presence_penalty) || !std::isfinite(frequency_penalty))
    return fail(SMX_ERR_INVALID, "presence_penalty and frequency_penalty must be finite");
  if (top_k < 0 || max_run_length < 0) return fail(SMX_ERR_INVALID, "top_k and max_run_length must not be negative");
  const SampleArgs a{temperature, top_p, repetition_penalty, presence_penalty, frequency_penalty,
                     top_k, ascii_only != 0, ban_cr != 0, max_run_length};
  HIP_TRY(launch_sample_bytes(logits, row_stride, recent, kind, n_recent, a, u, ids, probs, R, (hipStream_t)stream));
  return SMX_OK;
}

// ---- byte-spectral features (smx_byte.hip) -------------------------------------------------------------------------------
static int byte_shape(int B, const char* rows, int R, int W, int k) {
  if (B <= 0 || R <= 0 || W <= 0 || k < 0)
    return fail(SMX_ERR_INVALID, "shape must be positive (k: not negative): B=%d %s=%d W=%d", B, rows, R, W);
  return SMX_OK;
}
int smx_byte_supported(int T, int k, int W) { return byte_supported(T, k, W) ? 1 : 0; }
int smx_byte_features(const void* tokens, int token_bytes, long long row_stride, const float* bands, float* out,
                      float* mag, int B, int T, int k, int W, int P, void* stream) {
  if (int rc = byte_shape(B, "T", T, W, k)) return rc;
  if (P != 1 && P != T) return fail(SMX_ERR_INVALID, "P must be 1 (one row per sequence) or T=%d, got %d", T, P);
  if (k > T / 2) return fail(SMX_ERR_INVALID, "k must be at most T / 2: k=%d T=%d", k, T);
  if (!tokens || !out || (k > 0 && !bands)) return fail(SMX_ERR_INVALID, "tokens, out and (k > 0) bands must be non-NULL");
  int kind;
  if (int rc = token_src(tokens, token_bytes, row_stride, T, true, &kind)) return rc;
  if ((uintptr_t)out & 15) return fail(SMX_ERR_INVALID, "out must be 16-byte aligned");
  if (((uintptr_t)bands | (uintptr_t)mag) & 3) return fail(SMX_ERR_INVALID, "bands and mag must be 4-byte aligned");
  if (!byte_supported(T, k, W))
    return fail(SMX_ERR_UNSUPPORTED, "unsupported size (smx_byte_supported): T=%d k=%d W=%d", T, k, W);
  if ((long long)B * (P == 1 ? 1 : (T + 15) / 16) >= (1ll << 31) || (long long)B * P * W >= (1ll << 40))
    return fail(SMX_ERR_INVALID, "B*P*W too large");
  HIP_TRY(launch_byte_features(tokens, kind, row_stride, bands, out, mag, B, T, k, W, P, (hipStream_t)stream));
  return SMX_OK;
}
int smx_byte_workspace_bytes(int B, int P, int W, int k, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  if (int rc = byte_shape(B, "P", P, W, k)) return rc;
  *out = byte_gb_part_bytes(B, P, k < W ? k : W);
  return SMX_OK;
}
int smx_byte_grad_bands(const float* g, const float* mag, float* grad_bands, int n_bands, void* workspace,
                        size_t workspace_bytes, int B, int P, int W, int k, void* stream) {
  if (int rc = byte_shape(B, "P", P, W, k)) return rc;
  const int kk = k < W ? k : W;
  if (n_bands < kk || n_bands < 1) return fail(SMX_ERR_INVALID, "n_bands must be at least max(1, min(k, W)), got %d", n_bands);
  if (!g || !grad_bands || (kk > 0 && !mag)) return fail(SMX_ERR_INVALID, "g, grad_bands and (k > 0) mag must be non-NULL");
  if (((uintptr_t)g | (uintptr_t)mag | (uintptr_t)grad_bands) & 3) return fail(SMX_ERR_INVALID, "pointers must be 4-byte aligned");
  if (byte_gb_blocks(B, P, kk) >= (1ll << 31)) return fail(SMX_ERR_INVALID, "B*P too large");
  if (const size_t need = byte_gb_part_bytes(B, P, kk))      // (kk = 0: no partials, any workspace)
    if (int rc = need_ws(workspace, workspace_bytes, need, SMX_ERR_INVALID, nullptr, "smx_byte_workspace_bytes")) return rc;
  HIP_TRY(launch_byte_grad_bands(g, mag, (float*)workspace, grad_bands, n_bands, B, P, W, k, (hipStream_t)stream));
  return SMX_OK;
}

// ---- multi-pattern exact byte search (smx_match.hip) ---------------------------------------------------------------------
// (`max_workgroups` of this search, of the top-k passes and of the scatter: 0 = the launcher's own count)
static int wg_check(int max_workgroups) {
  if (max_workgroups < 0) return fail(SMX_ERR_INVALID, "max_workgroups must not be negative, got %d", max_workgroups);
  return SMX_OK;
}
static int match_check(int S, int L) {
  if (!match_supported(S, L))
    return fail(SMX_ERR_UNSUPPORTED, "unsupported snippet set (smx_match_supported): S=%d L=%d", S, L);
  return SMX_OK;
}
int smx_match_supported(int S, int L) { return match_supported(S, L) ? 1 : 0; }
int smx_match_workspace_bytes(int S, int L, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  if (int rc = match_check(S, L)) return rc;
  *out = match_part_bytes(S);
  return SMX_OK;
}
int smx_match_first(const void* corpus, long long n, const void* snips, int S, int L, long long* first, void* workspace,
                    size_t workspace_bytes, int max_workgroups, void* stream) {
  if (int rc = match_check(S, L)) return rc;
  if (n < 0) return fail(SMX_ERR_INVALID, "n must not be negative, got %lld", n);
  if (!snips || !first || (n > 0 && !corpus))
    return fail(SMX_ERR_INVALID, "corpus (n > 0), snips and first must be non-NULL");
  if ((uintptr_t)first & 7) return fail(SMX_ERR_INVALID, "first must be 8-byte aligned");
  if (int rc = wg_check(max_workgroups)) return rc;
  if (int rc = need_ws(workspace, workspace_bytes, match_part_bytes(S), SMX_ERR_WORKSPACE, nullptr, "smx_match_workspace_bytes"))
    return rc;
  HIP_TRY(launch_match_first((const unsigned char*)corpus, n, (const unsigned char*)snips, S, L, first,
                             (unsigned long long*)workspace, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}

// ---- top-k sparsify and scatter of the sparse spectral tensor (smx_sst.hip) ------------------------------------------------
static int topk_check(long long n) {
  if (!topk_supported(n)) return fail(SMX_ERR_UNSUPPORTED, "unsupported size (smx_topk_supported): n=%lld", n);
  return SMX_OK;
}
static int topk_ws(const char* who, long long n, const void* workspace, size_t workspace_bytes) {
  return need_ws(workspace, workspace_bytes, topk_layout(n).need, SMX_ERR_WORKSPACE, who, "smx_topk_workspace_bytes");
}
int smx_topk_supported(long long n) { return topk_supported(n) ? 1 : 0; }
int smx_topk_workspace_bytes(long long n, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  if (int rc = topk_check(n)) return rc;
  *out = topk_layout(n).need;
  return SMX_OK;
}
int smx_topk_select(const void* z, long long n, long long k, long long* result, void* workspace, size_t workspace_bytes,
                    int max_workgroups, void* stream) {
  if (int rc = topk_check(n)) return rc;
  if (!z || !result) return fail(SMX_ERR_INVALID, "z and result must be non-NULL");
  if (k < 1 || k > n) return fail(SMX_ERR_INVALID, "k must be in 1..n, got k=%lld n=%lld", k, n);
  if (((uintptr_t)z & 7) || ((uintptr_t)result & 7)) return fail(SMX_ERR_INVALID, "z and result must be 8-byte aligned");
  if (int rc = wg_check(max_workgroups)) return rc;
  if (int rc = topk_ws("smx_topk_select", n, workspace, workspace_bytes)) return rc;
  HIP_TRY(launch_topk_select((const float2*)z, n, k, result, workspace, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}
int smx_topk_compact(const void* z, long long n, const long long* result, void* coeffs, long long* flat_idx,
                     long long capacity, void* workspace, size_t workspace_bytes, int max_workgroups, void* stream) {
  if (int rc = topk_check(n)) return rc;
  if (capacity < 0) return fail(SMX_ERR_INVALID, "capacity must not be negative, got %lld", capacity);
  if (!z || !result || (capacity > 0 && (!coeffs || !flat_idx)))
    return fail(SMX_ERR_INVALID, "z, result and (capacity > 0) coeffs, flat_idx must be non-NULL");
  if (((uintptr_t)z & 7) || ((uintptr_t)result & 7) || ((uintptr_t)coeffs & 7) || ((uintptr_t)flat_idx & 7))
    return fail(SMX_ERR_INVALID, "z, result, coeffs and flat_idx must be 8-byte aligned");
  if (int rc = wg_check(max_workgroups)) return rc;
  if (int rc = topk_ws("smx_topk_compact", n, workspace, workspace_bytes)) return rc;
  if (capacity == 0) return SMX_OK;
  HIP_TRY(launch_topk_compact((const float2*)z, n, result, (float2*)coeffs, flat_idx, capacity, workspace, max_workgroups,
                              (hipStream_t)stream));
  return SMX_OK;
}
int smx_sparse_scatter(const void* coeffs, const long long* flat_idx, long long m, void* out, long long n,
                       int max_workgroups, void* stream) {
  if (int rc = topk_check(n)) return rc;
  if (m < 0 || m > n) return fail(SMX_ERR_INVALID, "m must be in 0..n, got m=%lld n=%lld", m, n);
  if (!out || (m > 0 && (!coeffs || !flat_idx)))
    return fail(SMX_ERR_INVALID, "out and (m > 0) coeffs, flat_idx must be non-NULL");
  if ((uintptr_t)out & 15) return fail(SMX_ERR_INVALID, "out must be 16-byte aligned");
  if (((uintptr_t)coeffs & 7) || ((uintptr_t)flat_idx & 7))
    return fail(SMX_ERR_INVALID, "coeffs and flat_idx must be 8-byte aligned");
  if (int rc = wg_check(max_workgroups)) return rc;
  HIP_TRY(launch_sparse_scatter((const float2*)coeffs, flat_idx, m, (float2*)out, n, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}

// ---- frequency attention and frequency layernorm (smx_freq.hip) -----------------------------------------------------------
static_assert(FREQ_LN_MAX_D == SMX_FREQ_LN_MAX_D, "smx_freq.h states the limit of smx_kernels.h");
// 0: run it, 1: zero-sized (success, nothing to enqueue), negative: refused
static int fattn_check(int B, int H, int N) {
  if (B < 0 || H < 0 || N < 0) return fail(SMX_ERR_INVALID, "sizes must not be negative: B=%d H=%d N=%d", B, H, N);
  if (B == 0 || H == 0 || N == 0) return 1;
  if ((long long)B * H * N >= (1ll << 31) || N > FATTN_MAX_N)
    return fail(SMX_ERR_UNSUPPORTED, "B*H*N must stay below 2^31 and N at or below 2^30: B=%d H=%d N=%d", B, H, N);
  return 0;
}
static size_t fattn_need(int B, int H, int N) { return WS_HEADER_BYTES + al((size_t)B * H * N * sizeof(float)); }
int smx_freq_attention_workspace_bytes(int B, int H, int N, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  const int rc = fattn_check(B, H, N);
  if (rc < 0) return rc;
  *out = rc ? 0 : fattn_need(B, H, N);
  return SMX_OK;
}
int smx_freq_attention_forward(const void* q, long long q_sb, long long q_sh, long long q_sn,
                               const void* k, long long k_sb, long long k_sh, long long k_sn,
                               const void* v, long long v_sb, long long v_sh, long long v_sn,
                               void* out, long long o_sb, long long o_sh, long long o_sn, float temperature,
                               void* workspace, size_t workspace_bytes, int B, int H, int N, int D, void* stream) {
  const int rc = fattn_check(B, H, N);
  if (rc < 0) return rc;
  if (D < 0) return fail(SMX_ERR_INVALID, "D must not be negative, got %d", D);
  FattnArgs a{};
  const long long st[12] = {q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn};
  for (int i = 0; i < 12; ++i) {
    if (st[i] < 0) return fail(SMX_ERR_INVALID, "strides must not be negative");
    (i < 3 ? a.sq : i < 6 ? a.sk : i < 9 ? a.sv : a.so)[i % 3] = st[i];
  }
  if (!std::isfinite(temperature) || temperature == 0.f)
    return fail(SMX_ERR_INVALID, "temperature must be finite and not 0, got %g", (double)temperature);
  if (rc || D == 0) return SMX_OK;
  if (!q || !k || !v || !out) return fail(SMX_ERR_INVALID, "q, k, v and out must be non-NULL");
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 7)
    return fail(SMX_ERR_INVALID, "q, k, v and out must be 8-byte aligned");
  if (need_ws(workspace, workspace_bytes, fattn_need(B, H, N), "smx_freq_attention_workspace_bytes")) return SMX_ERR_INVALID;
  if (!&launch_fattn) return fail(SMX_ERR_UNSUPPORTED, "this build holds no smx_freq unit");
  a.q = (const float2*)q; a.k = (const float2*)k; a.v = (const float2*)v; a.out = (float2*)out;
  a.rows = (long long)B * H * N; a.H = H; a.N = N; a.D = D;
  a.scale = (float)(1.0 / ((double)temperature * (double)D));
  HIP_TRY(launch_fattn(a, (float*)((char*)workspace + WS_HEADER_BYTES), (hipStream_t)stream));
  return SMX_OK;
}
int smx_freq_layernorm_forward(const void* z, void* out, float eps, long long rows, int D, void* stream) {
  if (rows < 0 || D < 0) return fail(SMX_ERR_INVALID, "sizes must not be negative: rows=%lld D=%d", rows, D);
  if (rows == 0 || D == 0) return SMX_OK;
  if (!z || !out) return fail(SMX_ERR_INVALID, "z and out must be non-NULL");
  if (((uintptr_t)z | (uintptr_t)out) & 15) return fail(SMX_ERR_INVALID, "z and out must be 16-byte aligned");
  if (!freq_ln_supported(D))
    return fail(SMX_ERR_UNSUPPORTED, "D=%d is wider than SMX_FREQ_LN_MAX_D=%d", D, SMX_FREQ_LN_MAX_D);
  if (rows >= (1ll << 40)) return fail(SMX_ERR_UNSUPPORTED, "rows must stay below 2^40");
  if (!&launch_freq_ln) return fail(SMX_ERR_UNSUPPORTED, "this build holds no smx_freq unit");
  HIP_TRY(launch_freq_ln((const float*)z, (float*)out, eps, rows, D, (hipStream_t)stream));
  return SMX_OK;
}

// ---- per-bin channel contraction of the FFT convolutions (smx_fconv.hip) ------------------------------------------------------
// 0: run it, 1: zero-sized (success, nothing to enqueue), negative: refused
static int bin_check(int B, long long P, int Ci, int Co, int max_workgroups) {
  if (B < 0 || P < 0 || Ci < 0 || Co < 0)
    return fail(SMX_ERR_INVALID, "sizes must not be negative: B=%d P=%lld Ci=%d Co=%d", B, P, Ci, Co);
  if (int rc = wg_check(max_workgroups)) return rc;
  if (B == 0 || P == 0 || Ci == 0 || Co == 0) return 1;
  if (!&bin_contract_supported || !&launch_bin_contract_fwd || !&launch_bin_contract_bwd)
    return fail(SMX_ERR_UNSUPPORTED, "this build holds no smx_fconv unit");
  if (!bin_contract_supported(B, P, Ci, Co))
    return fail(SMX_ERR_UNSUPPORTED, "unsupported size (smx_bin_contract_supported): B=%d P=%lld Ci=%d Co=%d", B, P, Ci, Co);
  return 0;
}
int smx_bin_contract_supported(int B, long long P, int Ci, int Co) {
  return &bin_contract_supported && bin_contract_supported(B, P, Ci, Co) ? 1 : 0;
}
int smx_bin_contract_forward(const void* x, const void* w, void* y, int B, long long P, int Ci, int Co, int max_workgroups,
                             void* stream) {
  const int rc = bin_check(B, P, Ci, Co, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!x || !w || !y) return fail(SMX_ERR_INVALID, "x, w and y must be non-NULL");
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 7) return fail(SMX_ERR_INVALID, "x, w and y must be 8-byte aligned");
  HIP_TRY(launch_bin_contract_fwd((const float2*)x, (const float2*)w, (float2*)y, B, P, Ci, Co, max_workgroups,
                                  (hipStream_t)stream));
  return SMX_OK;
}
int smx_bin_contract_backward(const void* x, const void* w, const void* gy, void* gx, void* gw, int B, long long P, int Ci,
                              int Co, int max_workgroups, void* stream) {
  const int rc = bin_check(B, P, Ci, Co, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!gx && !gw) return SMX_OK;
  if (!gy || (gx && !w) || (gw && !x))
    return fail(SMX_ERR_INVALID, "gy, w (for gx) and x (for gw) must be non-NULL");
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)gy | (uintptr_t)gx | (uintptr_t)gw) & 7)
    return fail(SMX_ERR_INVALID, "x, w, gy, gx and gw must be 8-byte aligned");
  HIP_TRY(launch_bin_contract_bwd((const float2*)x, (const float2*)w, (const float2*)gy, (float2*)gx, (float2*)gw, B, P, Ci,
                                  Co, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}

// ---- the polar and log8 codecs (smx_quant.hip) ----------------------------------------------------------------------------------
// 0: run it, 1: zero-sized (success, nothing to enqueue), negative: refused
static int quant_check(long long n, int max_workgroups) {
  if (n < 0) return fail(SMX_ERR_INVALID, "n must not be negative, got %lld", n);
  if (int rc = wg_check(max_workgroups)) return rc;
  return n == 0 ? 1 : 0;
}
static int quant_bits(int mag_bits, int phase_bits) {
  if (mag_bits < 1 || mag_bits > 8 || phase_bits < 1 || phase_bits > 8)
    return fail(SMX_ERR_INVALID, "mag_bits and phase_bits must be in 1..8, got %d and %d", mag_bits, phase_bits);
  return SMX_OK;
}
static int quant_unit(const void* launcher) {
  if (!launcher) return fail(SMX_ERR_UNSUPPORTED, "this build holds no smx_quant unit");
  return SMX_OK;
}
int smx_polar_range_workspace_bytes(long long n, size_t* out) {
  if (!out) return fail(SMX_ERR_INVALID, "out is NULL");
  if (n < 0) return fail(SMX_ERR_INVALID, "n must not be negative, got %lld", n);
  if (int rc = quant_unit((const void*)&quant_range_part_bytes)) return rc;
  *out = n == 0 ? 0 : quant_range_part_bytes();
  return SMX_OK;
}
int smx_polar_range(const void* z, long long n, void* out2, void* workspace, size_t workspace_bytes, int max_workgroups,
                    void* stream) {
  const int rc = quant_check(n, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!z || !out2) return fail(SMX_ERR_INVALID, "z and out2 must be non-NULL");
  if (((uintptr_t)z & 7) || ((uintptr_t)out2 & 3)) return fail(SMX_ERR_INVALID, "z must be 8-byte, out2 4-byte aligned");
  if (int r = quant_unit((const void*)&launch_polar_range)) return r;
  if (need_ws(workspace, workspace_bytes, quant_range_part_bytes(), "smx_polar_range_workspace_bytes")) return SMX_ERR_INVALID;
  HIP_TRY(launch_polar_range((const float2*)z, n, (float*)out2, (float2*)workspace, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}
int smx_polar_quantize(const void* z, void* mag_q, void* phase_q, long long n, int mag_bits, int phase_bits, float mag_min,
                       float mag_max, int max_workgroups, void* stream) {
  if (int r = quant_bits(mag_bits, phase_bits)) return r;
  const int rc = quant_check(n, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!z || !mag_q || !phase_q) return fail(SMX_ERR_INVALID, "z, mag_q and phase_q must be non-NULL");
  if ((uintptr_t)z & 7) return fail(SMX_ERR_INVALID, "z must be 8-byte aligned");
  if (int r = quant_unit((const void*)&launch_polar_quantize)) return r;
  HIP_TRY(launch_polar_quantize((const float2*)z, (unsigned char*)mag_q, (unsigned char*)phase_q, n, mag_bits, phase_bits,
                                mag_min, mag_max, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}
int smx_polar_dequantize(const void* mag_q, const void* phase_q, void* z, long long n, int mag_bits, int phase_bits,
                         float mag_min, float mag_max, int max_workgroups, void* stream) {
  if (int r = quant_bits(mag_bits, phase_bits)) return r;
  const int rc = quant_check(n, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!z || !mag_q || !phase_q) return fail(SMX_ERR_INVALID, "mag_q, phase_q and z must be non-NULL");
  if ((uintptr_t)z & 7) return fail(SMX_ERR_INVALID, "z must be 8-byte aligned");
  if (int r = quant_unit((const void*)&launch_polar_dequantize)) return r;
  HIP_TRY(launch_polar_dequantize((const unsigned char*)mag_q, (const unsigned char*)phase_q, (float2*)z, n, mag_bits,
                                  phase_bits, mag_min, mag_max, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}
int smx_log8_encode(const void* x, void* out, long long n, int max_workgroups, void* stream) {
  const int rc = quant_check(n, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!x || !out) return fail(SMX_ERR_INVALID, "x and out must be non-NULL");
  if ((uintptr_t)x & 3) return fail(SMX_ERR_INVALID, "x must be 4-byte aligned");
  if (int r = quant_unit((const void*)&launch_log8_encode)) return r;
  HIP_TRY(launch_log8_encode((const float*)x, (unsigned char*)out, n, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}
int smx_log8_decode(const void* e, void* x, long long n, int max_workgroups, void* stream) {
  const int rc = quant_check(n, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!e || !x) return fail(SMX_ERR_INVALID, "e and x must be non-NULL");
  if ((uintptr_t)x & 3) return fail(SMX_ERR_INVALID, "x must be 4-byte aligned");
  if (int r = quant_unit((const void*)&launch_log8_decode)) return r;
  HIP_TRY(launch_log8_decode((const unsigned char*)e, (float*)x, n, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}
int smx_log8_encode_c64(const void* z, void* re_q, void* im_q, long long n, int max_workgroups, void* stream) {
  const int rc = quant_check(n, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!z || !re_q || !im_q) return fail(SMX_ERR_INVALID, "z, re_q and im_q must be non-NULL");
  if ((uintptr_t)z & 7) return fail(SMX_ERR_INVALID, "z must be 8-byte aligned");
  if (int r = quant_unit((const void*)&launch_log8_encode_c64)) return r;
  HIP_TRY(launch_log8_encode_c64((const float2*)z, (unsigned char*)re_q, (unsigned char*)im_q, n, max_workgroups,
                                 (hipStream_t)stream));
  return SMX_OK;
}
int smx_log8_decode_c64(const void* re_q, const void* im_q, void* z, long long n, int max_workgroups, void* stream) {
  const int rc = quant_check(n, max_workgroups);
  if (rc) return rc < 0 ? rc : SMX_OK;
  if (!z || !re_q || !im_q) return fail(SMX_ERR_INVALID, "re_q, im_q and z must be non-NULL");
  if ((uintptr_t)z & 7) return fail(SMX_ERR_INVALID, "z must be 8-byte aligned");
  if (int r = quant_unit((const void*)&launch_log8_decode_c64)) return r;
  HIP_TRY(launch_log8_decode_c64((const unsigned char*)re_q, (const unsigned char*)im_q, (float2*)z, n, max_workgroups,
                                 (hipStream_t)stream));
  return SMX_OK;
}

// ---- the DFT along the contiguous last axis (smx_rowfft.hip) ------------------------------------------------------------------
int smx_rowfft_supported(int n) { return rowfft_supported(n) ? 1 : 0; }
int smx_rowfft(const void* in, void* out, long long rows, int n, int flags, float scale, int max_workgroups, void* stream) {
  if (rows < 0) return fail(SMX_ERR_INVALID, "rows must not be negative, got %lld", rows);
  if (int rc = wg_check(max_workgroups)) return rc;
  if (flags & ~(SMX_ROWFFT_CONJ_IN | SMX_ROWFFT_CONJ_OUT | SMX_ROWFFT_REAL_IN | SMX_ROWFFT_REAL_OUT))
    return fail(SMX_ERR_INVALID, "unknown flag bits in %d (SMX_ROWFFT_*)", flags);
  if (!std::isfinite(scale)) return fail(SMX_ERR_INVALID, "scale must be finite");
  if (!rowfft_supported(n))
    return fail(SMX_ERR_UNSUPPORTED, "n must be a power of two from 2 to %d (smx_rowfft_supported), got %d", SMX_ROWFFT_MAX_N, n);
  if (rows == 0) return SMX_OK;
  if (!in || !out) return fail(SMX_ERR_INVALID, "in and out must be non-NULL");
  if (((uintptr_t)in & 15) || ((uintptr_t)out & 15)) return fail(SMX_ERR_INVALID, "in and out must be 16-byte aligned");
  if (!(const void*)&launch_rowfft) return fail(SMX_ERR_UNSUPPORTED, "this build holds no smx_rowfft unit");
  HIP_TRY(launch_rowfft(in, out, rows, n, flags, scale, max_workgroups, (hipStream_t)stream));
  return SMX_OK;
}

}  // extern "C"
