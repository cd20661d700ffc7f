// launch_trace -- which kernel instance and grid every launcher of the transform families picks (CPU, no GPU).
//
// Built by build.sh with hipcc --cuda-host-only -DSMX_LAUNCH_TRACE together with the kernel translation units: under
// that switch SMX_LAUNCH (smx_launch.h) records instead of launching.  One line per launcher call, the inputs in the
// order of the launcher's `#` line:
//     <launcher> <value> ...: refused                                (the launcher returned an error)
//     <launcher> <value> ...: <instance> <grid.x>x<grid.y>x<block.x>@<bid0> | ...     (the launches, in order)
// tests/test_launch_trace.py compares the output with expected.txt.
//
// Inputs: every value a launcher's selection distinguishes plus one outside each range -- nb 1 2 4 3; mode 0 ... 3
// for the launchers with modes 0 1 2, 0 ... 5 for the column launches (modes 0 ... 4); io 0 ... 3; oio -1 ... 2; dir 0 1;
// nj 8 16; rows R < N or not (pad); drop_thr zero or not; accumulate; out null or not; ... -- as one cross
// product per launcher, with these cuts that keep expected.txt below 256 KiB:
//   * the grid inputs (a.round 0 / 512; 80 and 1280 workgroups: B = 40, D = 64 with nsplit 1 and 16, or B = 640) are
//     varied at a few settings of the selection inputs only, the selection inputs at round 0, B = 40, nsplit 1;
//   * launch_fused: out == NULL only changes the pick of an accumulating launch, so it is crossed with accumulate set;
//     beside io = 3 or oio = 1, 2 (no instance) pad / drop / acc are set one at a time.  The last column (n_cons) was
//     an input that no longer exists: it prints 0, so the lines keep their text;
//   * launch_fs_f: fs_bgroups and the row-scale gradient (gsc with gsc_part) only bear on mode 1 -- crossed there at
//     every L up to 64 and every multiple of 4 above, and with the other modes at L = 8, 18, 48, 64.
#include <cxxabi.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#include "smx_kernels.h"

namespace smx {
static std::string g_rec;
void trace_launch(const char* ktag, dim3 grid, dim3 block, const DecimArgs* a) {
  int st = 0;
  char* d = abi::__cxa_demangle(ktag, nullptr, nullptr, &st);
  std::string n = d ? d : ktag;
  free(d);
  // smx::KTag<&(void smx::k<1, 0, true>(smx::DecimArgs))> or smx::KTag<&smx::k>  ->  k<1, 0, true> / k
  for (size_t p; (p = n.find("smx::")) != std::string::npos;) n.erase(p, 5);
  for (size_t p; (p = n.find("(anonymous namespace)::")) != std::string::npos;) n.erase(p, 23);
  const size_t lt = n.find('<');
  if (lt != std::string::npos && n.size() > lt + 2) n = n.substr(lt + 1, n.size() - lt - 2);
  if (n.rfind("&(", 0) == 0 && n.back() == ')') n = n.substr(2, n.size() - 3);
  else if (n.rfind("&", 0) == 0) n.erase(0, 1);
  if (n.rfind("void ", 0) == 0) n.erase(0, 5);
  int depth = 0;                                   // drop the parameter list: the first '(' outside <...>
  for (size_t i = 0; i < n.size(); ++i) {
    if (n[i] == '<') ++depth;
    else if (n[i] == '>') --depth;
    else if (n[i] == '(' && depth == 0) { n.erase(i); break; }
  }
  char buf[96];
  for (size_t p; (p = n.find(", ")) != std::string::npos;) n.erase(p + 1, 1);
  if (a) snprintf(buf, sizeof buf, " %ux%ux%u@%d", grid.x, grid.y, block.x, a->bid0);
  else snprintf(buf, sizeof buf, " %ux%ux%u", grid.x, grid.y, block.x);
  if (!g_rec.empty()) g_rec += " |";
  g_rec += " " + n + buf;
}
}  // namespace smx

// The units' static constructors register their kernels with the HIP runtime; there is no code object to register
// (host-only compile), so the entry points end here and the runtime is never entered.
extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
}

using namespace smx;

template <class T> static T* dummy() { return reinterpret_cast<T*>(0x1000); }

// every pointer a dummy, the shape (B, R, D) at n_fft = N
static DecimArgs args(int B, int D, int N, int R, int nsplit = 1, int round = 0) {
  DecimArgs a{};
  a.in = dummy<float>(); a.out = dummy<float>(); a.tw = a.bt = a.tq = a.v16 = a.b16 = dummy<cf>();
  a.g.B = B; a.g.N = N; a.g.D = D; a.g.F = N / 2 + 1; a.g.k = N / 2 + 1; a.g.L = N / 256; a.g.inv_n = 1.f / N; a.g.R = R;
  a.fa.w_re = a.fa.w_im = a.fa.xk_in = dummy<float>(); a.fa.xk_out = a.fa.pslab = a.fa.gb_part = dummy<float>();
  a.placement = 2; a.round = round; a.st_plain = 4;
  a.nsplit = nsplit; a.lc = (a.g.L + nsplit - 1) / nsplit;
  a.ws_z = a.ws_zs = a.ws_s = a.ws_f = dummy<cf>(); a.conv_src = dummy<cf>();
  a.ca.h_re = a.ca.h_im = dummy<float>(); a.ca.xs = dummy<cf>(); a.ca.p_part = a.ca.r_part = dummy<cf>();
  a.drop_scale = 1.f; a.rng = dummy<unsigned long long>();
  a.ln_stats = dummy<cf>(); a.ln_w = a.ln_b = dummy<float>();
  return a;
}

static char g_in[512];
#define IN(...) snprintf(g_in, sizeof g_in, __VA_ARGS__)
template <class F>
static void call(F f) {
  g_rec.clear();
  const hipError_t e = f();
  if (e != hipSuccess) printf("%s: refused%s%s\n", g_in, g_rec.empty() ? "" : " after", g_rec.c_str());
  else printf("%s:%s\n", g_in, g_rec.empty() ? " nothing" : g_rec.c_str());
}

static const int NBS[] = {1, 2, 4, 3}, MODES3[] = {0, 1, 2, 3}, MODES5[] = {0, 1, 2, 3, 4, 5}, IOS[] = {0, 1, 2, 3},
                 OIOS[] = {-1, 0, 1, 2};
static const hipStream_t S = nullptr;
constexpr int N0 = 1024;
constexpr unsigned THR = 6554;            // dropout p = 0.1

// ---- the grid shapes at D = 64: GRIDS[0] is where the selection inputs are varied ---------------------------------
struct GridCase { int B, nsplit, round; };
static const GridCase GRIDS[] = {{40, 1, 0}, {40, 1, 512}, {40, 16, 0}, {40, 16, 512}, {640, 1, 0}, {640, 1, 512}};

static void fused() {
  puts("# fused: B round nb mode io oio pad drop acc out n_cons");
  auto one = [](const GridCase& gc, int nb, int mode, int io, int oio, int pad, int drop, int acc, int out) {
    DecimArgs a = args(gc.B, 64, N0, pad ? N0 / 2 : N0, 1, gc.round);
    a.drop_thr = drop ? THR : 0; a.accumulate = acc;
    if (!out) a.out = nullptr;
    IN("fused %d %d %d %d %d %d %d %d %d %d 0", gc.B, gc.round, nb, mode, io, oio, pad, drop, acc, out);
    call([&] { return launch_fused(a, nb, mode, S, io, oio); });
  };
  for (int nb : NBS) for (int mode : MODES3) for (int io : IOS) for (int oio : OIOS)
    for (int pad = 0; pad < 2; ++pad) for (int drop = 0; drop < 2; ++drop) for (int acc = 0; acc < 2; ++acc) {
      if ((io == 3 || oio > 0) && pad + drop + acc > 1) continue;       // beside a value no instance has: one at a time
      one(GRIDS[0], nb, mode, io, oio, pad, drop, acc, 1);
    }
  for (int nb : NBS) for (int mode : MODES3) for (int io : IOS) for (int pad = 0; pad < 2; ++pad)
    for (int drop = 0; drop < 2; ++drop) one(GRIDS[0], nb, mode, io, -1, pad, drop, 1, 0);
  // grid: rounds, the single launch of the four-band instances
  for (const GridCase& gc : GRIDS)
    if (gc.nsplit == 1 && &gc != &GRIDS[0])
      for (int nb : {1, 4}) for (int acc = 0; acc < 2; ++acc) one(gc, nb, 1, 0, -1, 0, 0, acc, 1);
}

static void fused16() {
  puts("# fused16: B round nb mode pad drop");
  for (const GridCase& gc : GRIDS) {
    if (gc.nsplit != 1) continue;
    for (int nb : NBS) for (int mode : MODES3) for (int pad = 0; pad < 2; ++pad) for (int drop = 0; drop < 2; ++drop) {
      if (&gc != &GRIDS[0] && (nb != 1 || mode != 0 || pad || drop)) continue;
      DecimArgs a = args(gc.B, 64, N0, pad ? N0 / 2 : N0, 1, gc.round);
      a.drop_thr = drop ? THR : 0;
      IN("fused16 %d %d %d %d %d %d", gc.B, gc.round, nb, mode, pad, drop);
      call([&] { return launch_fused16(a, nb, mode, S); });
    }
  }
}

// launchers of the shape f(a, nb, bool drop, s[, io]) over n_wg * nsplit workgroups; dflag = the bool, drop = drop_thr != 0
template <class F>
static void split_family(const char* name, bool with_io, F f) {
  printf("# %s: B nsplit round nb io dflag drop pad acc\n", name);
  for (const GridCase& gc : GRIDS)
    for (int nb : NBS) for (int io : IOS) for (int dflag = 0; dflag < 2; ++dflag) for (int drop = 0; drop < 2; ++drop)
      for (int pad = 0; pad < 2; ++pad) for (int acc = 0; acc < 2; ++acc) {
        if (!with_io && (io != 0 || acc)) continue;                  // (the sixteen-row launches take neither)
        if (&gc != &GRIDS[0] && (nb != 1 || io || dflag || drop || pad || acc)) continue;
        DecimArgs a = args(gc.B, 64, N0, pad ? N0 / 2 : N0, gc.nsplit, gc.round);
        a.drop_thr = drop ? THR : 0; a.accumulate = acc;
        IN("%s %d %d %d %d %d %d %d %d %d", name, gc.B, gc.nsplit, gc.round, nb, io, dflag, drop, pad, acc);
        call([&] { return f(a, nb, dflag != 0, io); });
      }
}

static void decim_rest() {
  puts("# synth: B round nb pad");
  for (const GridCase& gc : GRIDS)
    for (int nb : NBS) for (int pad = 0; pad < 2; ++pad) {
      if (gc.nsplit != 1 || (&gc != &GRIDS[0] && pad)) continue;
      DecimArgs a = args(gc.B, 64, N0, pad ? N0 / 2 : N0, 1, gc.round);
      IN("synth %d %d %d %d", gc.B, gc.round, nb, pad);
      call([&] { return launch_synth(a, nb, S); });
    }
  puts("# fused_block: B round nb io drop pad acc");
  for (const GridCase& gc : GRIDS)
    for (int nb : NBS) for (int io : IOS) for (int drop = 0; drop < 2; ++drop) for (int pad = 0; pad < 2; ++pad)
      for (int acc = 0; acc < 2; ++acc) {
        if (gc.nsplit != 1 || (&gc != &GRIDS[0] && (io || drop || pad || acc))) continue;
        DecimArgs a = args(gc.B, 64, N0, pad ? N0 / 2 : N0, 1, gc.round);
        a.drop_thr = drop ? THR : 0; a.accumulate = acc;
        IN("fused_block %d %d %d %d %d %d %d", gc.B, gc.round, nb, io, drop, pad, acc);
        call([&] { return launch_fused_block(a, nb, S, io); });
      }
  puts("# synth8: B round pad\n# full8: B round mode pad");
  for (const GridCase& gc : GRIDS)
    for (int pad = 0; pad < 2; ++pad) {
      if (gc.nsplit != 1) continue;
      DecimArgs a = args(gc.B, 64, 2048, pad ? 1024 : 2048, 1, gc.round);
      IN("synth8 %d %d %d", gc.B, gc.round, pad);
      call([&] { return launch_synth8(a, S); });
      for (int mode : MODES3) {
        IN("full8 %d %d %d %d", gc.B, gc.round, mode, pad);
        call([&] { return launch_full8(a, mode, S); });
      }
    }
  puts("# split_f: B nb mode sum_in_f");
  for (int B : {40, 640}) for (int nb : NBS) for (int mode : MODES3) for (int sum = 0; sum < 2; ++sum) {
    DecimArgs a = args(B, 64, N0, N0, 4, 0);
    a.sum_in_f = sum;
    IN("split_f %d %d %d %d", B, nb, mode, sum);
    call([&] { return launch_split_f(a, nb, mode, S); });
  }
}

static void conv1() {
  puts("# conv1: B N nj dir io R grad_scale");
  for (int B : {40, 640}) for (int N : {512, 1024, 2048, 4096}) for (int nj : {8, 16}) for (int dir = 0; dir < 2; ++dir)
    for (int io : IOS) for (int r4 = 1; r4 <= 4; ++r4) for (int gs = 0; gs < 2; ++gs) {     // R = N/4, N/2, 3N/4, N
      if (B != 40 && (N != 512 || io || r4 != 4)) continue;
      if (gs && !dir) continue;                                                     // grad_scale: backward only
      DecimArgs a = args(B, 64, N, N * r4 / 4);
      IN("conv1 %d %d %d %d %d %d %d", B, N, nj, dir, io, a.g.R, gs);
      call([&] { return launch_conv1(a, nj, dir, dummy<float>(), dummy<float>(), gs ? dummy<float>() : nullptr, S, io); });
    }
}

static void fourstep() {
  puts("# fs_a, fs_b: B nsplit round pad");
  for (const GridCase& gc : GRIDS) for (int pad = 0; pad < 2; ++pad) {
    DecimArgs a = args(gc.B, 64, 4096, pad ? 2048 : 4096, gc.nsplit, gc.round);
    IN("fs_a %d %d %d %d", gc.B, gc.nsplit, gc.round, pad);
    call([&] { return launch_fs_a(a, S); });
    IN("fs_b %d %d %d %d", gc.B, gc.nsplit, gc.round, pad);
    call([&] { return launch_fs_b(a, S); });
  }
  puts("# fs_f: B L mode fs_bgroups gsc");
  for (int L = 1; L <= 260; ++L) for (int mode : MODES5) for (int bg : {0, 8}) for (int gsc = 0; gsc < 2; ++gsc) {
    if (mode != 1 && (bg || gsc) && L != 8 && L != 18 && L != 48 && L != 64) continue;
    if ((bg || gsc) && L > 64 && L % 4 != 0) continue;               // (no two-level split: L2 = 4, 8 or 16 divides L)
    DecimArgs a = args(40, 64, 256 * L, 256 * L);
    a.fs_bgroups = bg;
    a.fa.gsc = gsc ? dummy<float>() : nullptr; a.fa.gsc_part = gsc ? dummy<cf>() : nullptr;
    IN("fs_f 40 %d %d %d %d", L, mode, bg, gsc);
    call([&] { return launch_fs_f(a, mode, S); });
  }
  for (int L : {8, 64, 48}) for (int gsc = 0; gsc < 2; ++gsc) {
    DecimArgs a = args(640, 64, 256 * L, 256 * L);
    a.fa.gsc = gsc ? dummy<float>() : nullptr; a.fa.gsc_part = gsc ? dummy<cf>() : nullptr;
    IN("fs_f 640 %d 1 0 %d", L, gsc);
    call([&] { return launch_fs_f(a, 1, S); });
  }
  puts("# fs_big_general: l1 l2 mode");
  for (int l1 = 8; l1 <= 17; ++l1) for (int l2 : {2, 4, 8, 16, 32}) for (int mode : MODES5) {
    DecimArgs a = args(40, 64, 256 * l1 * l2, 256 * l1 * l2);
    IN("fs_big_general %d %d %d", l1, l2, mode);
    call([&] { return launch_fs_big_general(a, mode, l1, l2, S); });
  }
  puts("# fs_conv: B L dir grad_scale");
  for (int B : {40, 640}) for (int L = 1; L <= 512; L *= 2) for (int dir = 0; dir < 2; ++dir) for (int gs = 0; gs < 2; ++gs) {
    if (gs && !dir) continue;
    DecimArgs a = args(B, 64, 256 * L, 256 * L);
    IN("fs_conv %d %d %d %d", B, L, dir, gs);
    call([&] { return launch_fs_conv(a, dir, dummy<float>(), dummy<float>(), gs ? dummy<float>() : nullptr, S); });
  }
}

int main() {
  fused();
  fused16();
  split_family("split16_a", false, [](const DecimArgs& a, int nb, bool d, int) { return launch_split16_a(a, nb, d, S); });
  split_family("split16_b", false, [](const DecimArgs& a, int nb, bool d, int) { return launch_split16_b(a, nb, d, S); });
  split_family("split_a", true, [](const DecimArgs& a, int nb, bool d, int io) { return launch_split_a(a, nb, d, S, io); });
  split_family("split_b", true, [](const DecimArgs& a, int nb, bool d, int io) { return launch_split_b(a, nb, d, S, io); });
  decim_rest();
  conv1();
  fourstep();
  return 0;
}
