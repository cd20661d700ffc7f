// api_trace -- what every C ABI entry of the library does with its arguments: return code, error text, and the
// launches in order (CPU, no GPU).
//
// Built by build.sh: the library's translation units compiled for the host alone, unchanged, and linked with this
// program, which defines the HIP runtime symbols the library calls -- the executable's definitions take precedence over
// libamdhip64's, so a launch ends in hipLaunchKernel below and is recorded.  One line per API call:
//     <entry> <inputs> -> <rc> <text of smx_last_error()> [after <launches>]            (rc != 0)
//     <entry> <inputs> -> 0: <kernel> <grid.x>[x<grid.y>[x<grid.z>]]/<block.x> #<digest> | ...
// (trailing grid dimensions of 1 are left out; "#=" is the digest of the launch before it in the line)
// (a launch with dynamic LDS: " lds=<bytes>" after the block)
// The digest is a 64-bit hash of the launch's arguments printed value by value (DecimArgs, DirectArgs, ByteArgs,
// MatchArgs, TopkArgs and SampleArgs field by field); --verbose prints those values instead (to read a mismatch; not compared).  Pointers are written
// symbolically -- ws+<offset>, tables:<bytes>.<n>+<offset> (the n-th allocation of its API call, <bytes> long), or the
// name of the dummy input -- so that a line depends neither on the allocator nor on the order of the calls (every
// n_fft is prepared by its own smx_prepare call before its first use).
// tests/test_api_trace.py compares the output with expected.txt, line for line.
//
// Sections: the plans over a grid of shapes and options; the transform entries on every plan kind; their call variants
// and options; block entries; convolution; the smaller ops; refusals, one fault at a time; the newer ops (word targets,
// row head, cross-entropy, sampler, byte features, byte search, top-k and scatter) with theirs.
#include <cxxabi.h>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "smx.h"
#include "smx_kernels.h"

using smx::DecimArgs;
using smx::DirectArgs;
using smx::ByteArgs;
using smx::MatchArgs;
using smx::SampleArgs;
using smx::TopkArgs;

// ---- symbolic addresses ----------------------------------------------------------------------------------------------
static constexpr uintptr_t DUMMY0 = 0x100000000000ull, DUMMY_SPAN = 1ull << 32, TAB0 = 0x200000000000ull,
                           WS0 = 0x400000000000ull, WS_SPAN = 1ull << 44;
static std::vector<std::string>& dummies() { static std::vector<std::string> v; return v; }
template <class T = float>
static T* dp(const char* name, int off = 0) {
  auto& v = dummies();
  size_t i = 0;
  while (i < v.size() && v[i] != name) ++i;
  if (i == v.size()) v.push_back(name);
  return reinterpret_cast<T*>(DUMMY0 + i * DUMMY_SPAN + off);
}
struct Alloc { uintptr_t base; size_t bytes; int ord; };
static std::vector<Alloc> g_allocs;
static uintptr_t g_bump = TAB0;
static int g_call_allocs = 0;

static std::string fmt(const char* f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}
static std::string sym(const void* ptr) {
  const uintptr_t p = (uintptr_t)ptr;
  if (!p) return "0";
  if (p >= WS0 && p < WS0 + WS_SPAN) return fmt("ws+%zu", (size_t)(p - WS0));
  if (p >= TAB0 && p < WS0) {
    for (const Alloc& a : g_allocs)
      if (p >= a.base && p < a.base + a.bytes) return fmt("tables:%zu.%d+%zu", a.bytes, a.ord, (size_t)(p - a.base));
    return "tables:?";
  }
  if (p >= DUMMY0 && p < DUMMY0 + dummies().size() * DUMMY_SPAN) {
    const size_t i = (p - DUMMY0) / DUMMY_SPAN, off = (p - DUMMY0) % DUMMY_SPAN;
    return off ? fmt("%s+%zu", dummies()[i].c_str(), off) : dummies()[i];
  }
  return fmt("?%zx", (size_t)p);
}

// ---- the record of one API call --------------------------------------------------------------------------------------
static std::string g_rec;
static bool g_verbose = false, g_capturing = false;
static unsigned long long g_last_digest = 0;
static void record(const std::string& head, const std::string& values) {
  if (!g_rec.empty()) g_rec += " | ";
  g_rec += head;
  if (values.empty()) return;
  if (g_verbose) { g_rec += " {" + values + " }"; return; }
  unsigned long long h = 1469598103934665603ull;            // FNV-1a
  for (unsigned char c : values) { h ^= c; h *= 1099511628211ull; }
  g_rec += h == g_last_digest ? std::string(" #=") : fmt(" #%016llx", h);
  g_last_digest = h;
}

// (" fa.slab_agent=0" and " sync=0 n_cons=0 gw_re=0 gw_im=0 gbias=0" are the text of fields that DecimArgs had until the
// folded parameter-gradient reduction was retired; no default launch ever set them, so the digests keep their values)
static std::string dump(const DecimArgs& a) {
  std::string s;
#define PTR(f) s += " " #f "=" + sym(a.f)
#define INT(f) s += fmt(" " #f "=%lld", (long long)a.f)
#define FLT(f) s += fmt(" " #f "=%.9g", (double)a.f)
  PTR(in); PTR(out); PTR(tw); PTR(bt); PTR(tq);
  INT(g.B); INT(g.N); INT(g.D); INT(g.F); INT(g.k); INT(g.L); FLT(g.inv_n); INT(g.R); INT(g.P); INT(g.st_plain);
  PTR(fa.w_re); PTR(fa.w_im); PTR(fa.wt); PTR(fa.bias); PTR(fa.xk_out); PTR(fa.xk_in); PTR(fa.pslab); PTR(fa.gb_part);
  INT(fa.conj_w); s += " fa.slab_agent=0"; PTR(fa.sc); PTR(fa.gsc); PTR(fa.gsc_part); INT(fa.goff); INT(fa.multi);
  FLT(fa.sp_scale); INT(fa.sp_herm);
  PTR(v16); PTR(b16); INT(placement); INT(accumulate); INT(round); INT(st_plain); INT(st_mask); INT(st_rsh); INT(st_wsh);
  INT(bid0); INT(nsplit); INT(lc); INT(sum_in_f); PTR(ws_z); PTR(ws_zs); PTR(ws_s); PTR(out_scale);
  PTR(ca.h_re); PTR(ca.h_im); PTR(ca.sc); PTR(ca.xs); PTR(ca.p_part); PTR(ca.r_part);
  PTR(conv_src); INT(fs_bgroups); PTR(ws_f); INT(drop_thr); FLT(drop_scale); PTR(rng);
  s += " sync=0 n_cons=0 gw_re=0 gw_im=0 gbias=0"; PTR(ln_stats); PTR(ln_w); PTR(ln_b);
  return s;
}
static std::string dump(const DirectArgs& a) {
  std::string s;
  INT(B); INT(N); INT(D); INT(F); INT(k); PTR(tw); INT(f0); INT(fstep); INT(rows); INT(accumulate); INT(R);
  return s;
}
static std::string dump(const ByteArgs& a) {
  std::string s;
  PTR(tokens); INT(row_stride); PTR(bands); PTR(out); PTR(mag); INT(B); INT(T); INT(k); INT(W); INT(P);
  INT(pp); INT(chunks); INT(ns_log); INT(cw_log);
  return s;
}
static std::string dump(const MatchArgs& a) {
  std::string s;
  PTR(corpus); PTR(snips); PTR(part); INT(n); INT(npos); INT(ntiles); INT(S); INT(L); INT(off); INT(nvec);
  return s;
}
static std::string dump(const TopkArgs& a) {
  std::string s;
  PTR(z); INT(n); INT(ntiles); INT(off);
  return s;
}
static std::string dump(const SampleArgs& a) {
  std::string s;
  FLT(temperature); FLT(top_p); FLT(rep); FLT(presence); FLT(frequency); INT(top_k); INT(ascii_only); INT(ban_cr);
  INT(max_run);
#undef PTR
#undef INT
#undef FLT
  return s;
}

// ---- kernels: host stub -> name and parameter types ------------------------------------------------------------------
struct Kernel { std::string name; std::vector<std::string> params; };
static std::map<const void*, Kernel>& kernels() { static std::map<const void*, Kernel> m; return m; }
static void strip(std::string& n, const char* what) {
  for (size_t p; (p = n.find(what)) != std::string::npos;) n.erase(p, strlen(what));
}
static Kernel parse_kernel(const char* mangled) {
  int st = 0;
  char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
  std::string n = d ? d : mangled;
  free(d);
  strip(n, "smx::"); strip(n, "(anonymous namespace)::");
  if (n.rfind("void ", 0) == 0) n.erase(0, 5);
  Kernel k;
  int depth = 0;
  size_t open = std::string::npos;                          // the parameter list: the first '(' outside <...>
  for (size_t i = 0; i < n.size() && open == std::string::npos; ++i) {
    if (n[i] == '<') ++depth;
    else if (n[i] == '>') --depth;
    else if (n[i] == '(' && depth == 0) open = i;
  }
  k.name = n.substr(0, open);
  for (size_t p; (p = k.name.find(", ")) != std::string::npos;) k.name.erase(p + 1, 1);
  if (open == std::string::npos) return k;
  std::string cur;
  depth = 0;
  for (size_t i = open + 1; i + 1 < n.size(); ++i) {
    const char c = n[i];
    if (c == '<' || c == '(') ++depth;
    if (c == '>' || c == ')') --depth;
    if (c == ',' && depth == 0) { k.params.push_back(cur); cur.clear(); ++i; continue; }
    cur += c;
  }
  if (!cur.empty()) k.params.push_back(cur);
  return k;
}

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void* host_fun, char*, const char* device_name, unsigned, void*, void*, void*,
                           void*, int*) {
  kernels()[host_fun] = parse_kernel(device_name);
}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
}
static dim3 g_grid, g_block;
static size_t g_shmem;
static hipStream_t g_stream;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t s) {
  g_grid = grid; g_block = block; g_shmem = shmem; g_stream = s;
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* s) {
  *grid = g_grid; *block = g_block; *shmem = g_shmem; *s = g_stream;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t) {
  auto it = kernels().find(f);
  if (it == kernels().end()) { record("unregistered-kernel", ""); return hipSuccess; }
  const Kernel& k = it->second;
  std::string v;
  for (size_t i = 0; i < k.params.size(); ++i) {
    const std::string& t = k.params[i];
    const void* a = args[i];
    if (t == "DecimArgs") v += dump(*(const DecimArgs*)a);
    else if (t == "DirectArgs") v += dump(*(const DirectArgs*)a);
    else if (t == "ByteArgs") v += dump(*(const ByteArgs*)a);
    else if (t == "MatchArgs") v += dump(*(const MatchArgs*)a);
    else if (t == "TopkArgs") v += dump(*(const TopkArgs*)a);
    else if (t == "SampleArgs") v += dump(*(const SampleArgs*)a);
    else if (t.back() == '*') v += " " + sym(*(void* const*)a);
    else if (t == "int") v += fmt(" %d", *(const int*)a);
    else if (t == "unsigned int") v += fmt(" %u", *(const unsigned*)a);
    else if (t == "long long" || t == "long") v += fmt(" %lld", *(const long long*)a);
    else if (t == "unsigned long long" || t == "unsigned long") v += fmt(" %llu", *(const unsigned long long*)a);
    else if (t == "float") v += fmt(" %.9g", (double)*(const float*)a);
    else if (t == "bool") v += fmt(" %d", (int)*(const bool*)a);
    else v += " (" + t + ")";
  }
  const std::string dims = grid.z > 1 ? fmt("%ux%ux%u", grid.x, grid.y, grid.z) : grid.y > 1 ? fmt("%ux%u", grid.x, grid.y) : fmt("%u", grid.x);
  record(k.name + " " + dims + fmt("/%u", block.x) + (lds ? fmt(" lds=%zu", lds) : std::string()), v);
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) {
  g_allocs.push_back({g_bump, bytes, g_call_allocs++});
  *p = (void*)g_bump;
  g_bump += (bytes + 4095) & ~(size_t)4095;
  return hipSuccess;
}
hipError_t hipFree(void*) { return hipSuccess; }
hipError_t hipMemcpy(void*, const void*, size_t, hipMemcpyKind) { return hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
  record("memset " + sym(dst) + fmt(" %d %zu", value, bytes), "");
  return hipSuccess;
}
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) {
  *st = g_capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
  return hipSuccess;
}

// ---- calls -----------------------------------------------------------------------------------------------------------
static char g_in[512];
#define IN(...) snprintf(g_in, sizeof g_in, __VA_ARGS__)
template <class F>
static void call(F f) {
  g_rec.clear();
  g_last_digest = 0;
  g_call_allocs = 0;
  const int rc = f();
  if (rc) printf("%s -> %d %s%s%s\n", g_in, rc, smx_last_error(), g_rec.empty() ? "" : " after ", g_rec.c_str());
  else printf("%s -> 0: %s\n", g_in, g_rec.empty() ? "nothing" : g_rec.c_str());
}
static void prepare(int N) {
  static std::set<int> done;
  if (!done.insert(N).second) return;
  g_call_allocs = 0;
  if (smx_prepare(N)) { printf("smx_prepare(%d) failed: %s\n", N, smx_last_error()); exit(1); }
}

// options of the calling context: the member ones through smx_options_push, the process-wide ones through smx_set_option
struct Opts {
  std::string name = "default";
  std::function<void(smx_options&)> set = [](smx_options&) {};
  const char* global = nullptr;
  int gvalue = 0;
};
struct Scope {
  const Opts o;
  explicit Scope(const Opts& opts) : o(opts) {
    smx_options v;
    smx_options_default(&v);
    o.set(v);
    smx_options_push(&v);
    if (o.global) smx_set_option(o.global, o.gvalue);
  }
  ~Scope() {
    smx_options_pop();
    if (o.global) smx_set_option(o.global, -2);      // (only the st_layout options are set this way: -2 = default)
  }
};
#define OPT(nm, stmt) Opts{nm, [](smx_options& o) { stmt; }}

static smx_shape layer(int B, int N, int D, int F) { return smx_shape{B, N, D, F, N, F < N / 2 ? F : N / 2}; }
static bool is_layer(const smx_shape& h) { return h.rows == h.n_fft && h.k == (h.F < h.n_fft / 2 ? h.F : h.n_fft / 2); }
static std::string shp(const smx_shape& h) { return fmt("(%d,%d,%d,F%d,N%d,k%d)", h.B, h.rows, h.D, h.F, h.n_fft, h.k); }
// ... in the input part of a line: `"` where it is the shape of the line above (sections start afresh)
static std::string g_last_shape;
static std::string shp_in(const smx_shape& h) {
  const std::string v = shp(h);
  if (v == g_last_shape) return "\"";
  g_last_shape = v;
  return v;
}
static void* const WS = (void*)WS0;
static size_t ws_bytes(const smx_shape& h) {
  size_t n = 0;
  return smx_workspace_bytes_ex(&h, &n) ? 1 << 20 : n;        // (a refused shape: any size)
}
static const unsigned long long* RNG() { return dp<unsigned long long>("rng"); }

// ---- the transform entries: one struct of arguments per entry, changed one member at a time ----------------------------
struct Fwd {
  const float *x = dp("x"), *w_re = dp("w_re"), *w_im = dp("w_im"), *bias = dp("bias");
  float *y = dp("y"), *xk = dp("xk");
  void* ws = WS;
  long long ws_delta = 0;              // bytes beside the queried size
  int conj_w = 0;
  float p = 0.f;
  const void* rng = RNG();
  float* pack = nullptr;
  const float* row_scale = nullptr;
  int io = -1;                         // >= 0: the _io entry
  bool ex = false;                     // the _ex entry (taken as well when the shape is not a layer shape)
};
static void fwd(const std::string& what, const smx_shape& h, const Fwd& a) {
  prepare(h.n_fft);
  const size_t wb = ws_bytes(h) + a.ws_delta;
  const bool ex = a.ex || !is_layer(h) || a.row_scale;
  IN("%s %s %s", a.io >= 0 ? "forward_io" : ex ? "forward_ex" : "forward_dropout", shp_in(h).c_str(), what.c_str());
  call([&] {
    if (a.io >= 0)
      return smx_forward_io(a.x, a.w_re, a.w_im, a.bias, a.y, a.xk, a.ws, wb, h.B, h.n_fft, h.D, h.F, a.conj_w, a.p,
                            a.rng, a.pack, nullptr, a.io);
    if (ex) return smx_forward_ex(&h, a.x, a.w_re, a.w_im, a.bias, a.y, a.xk, a.ws, wb, a.conj_w, a.pack, a.row_scale, nullptr);
    return smx_forward_dropout(a.x, a.w_re, a.w_im, a.bias, a.y, a.xk, a.ws, wb, h.B, h.n_fft, h.D, h.F, a.conj_w, a.p,
                               a.rng, a.pack, nullptr);
  });
}
struct Bwd {
  const float *g = dp("g"), *xk = dp("xk"), *w_re = dp("w_re"), *w_im = dp("w_im");
  float *grad_x = dp("grad_x"), *gw_re = dp("gw_re"), *gw_im = dp("gw_im"), *gbias = dp("gbias");
  void* ws = WS;
  long long ws_delta = 0;
  int phases = 7;
  float p = 0.f;
  const void* rng = RNG();
  const float* pack = nullptr;
  const float* row_scale = nullptr;
  float* grad_row_scale = nullptr;
  int io = -1;
  bool ex = false;
};
static void bwd(const std::string& what, const smx_shape& h, const Bwd& a) {
  prepare(h.n_fft);
  const size_t wb = ws_bytes(h) + a.ws_delta;
  const bool ex = a.ex || !is_layer(h) || a.row_scale || a.grad_row_scale;
  IN("%s %s %s", a.io >= 0 ? "backward_io" : ex ? "backward_ex" : "backward_dropout", shp_in(h).c_str(), what.c_str());
  call([&] {
    if (a.io >= 0)
      return smx_backward_io(a.g, a.xk, a.w_re, a.w_im, a.grad_x, a.gw_re, a.gw_im, a.gbias, a.ws, wb, h.B, h.n_fft, h.D,
                             h.F, a.phases, a.p, a.rng, a.pack, nullptr, a.io);
    if (ex)
      return smx_backward_ex(&h, a.g, a.xk, a.w_re, a.w_im, a.grad_x, a.gw_re, a.gw_im, a.gbias, a.ws, wb, a.phases,
                             a.pack, a.row_scale, a.grad_row_scale, nullptr);
    return smx_backward_dropout(a.g, a.xk, a.w_re, a.w_im, a.grad_x, a.gw_re, a.gw_im, a.gbias, a.ws, wb, h.B, h.n_fft,
                                h.D, h.F, a.phases, a.p, a.rng, a.pack, nullptr);
  });
}
struct Pair { const float* x = dp("x"); float* spec = dp("xk"); float* y = dp("y"); void* ws = WS; long long ws_delta = 0;
              float scale = 1.f; int herm = 0; };
static void spectrum(const std::string& what, const smx_shape& h, const Pair& a) {
  prepare(h.n_fft);
  const size_t wb = ws_bytes(h) + a.ws_delta;
  IN("%s %s %s", is_layer(h) ? "spectrum" : "spectrum_ex", shp_in(h).c_str(), what.c_str());
  call([&] {
    return is_layer(h) ? smx_spectrum(a.x, a.spec, a.ws, wb, h.B, h.n_fft, h.D, h.F, nullptr)
                       : smx_spectrum_ex(&h, a.x, a.spec, a.ws, wb, nullptr);
  });
}
static void rfft(const std::string& what, const smx_shape& h, const Pair& a) {
  prepare(h.n_fft);
  const size_t wb = ws_bytes(h) + a.ws_delta;
  IN("rfft_ex %s %s scale=%g herm=%d", shp_in(h).c_str(), what.c_str(), (double)a.scale, a.herm);
  call([&] { return smx_rfft_ex(&h, a.x, a.spec, a.scale, a.herm, a.ws, wb, nullptr); });
}
static void irfft(const std::string& what, const smx_shape& h, const Pair& a) {
  prepare(h.n_fft);
  const size_t wb = ws_bytes(h) + a.ws_delta;
  IN("irfft_ex %s %s scale=%g herm=%d", shp_in(h).c_str(), what.c_str(), (double)a.scale, a.herm);
  call([&] { return smx_irfft_ex(&h, a.spec, a.y, a.scale, a.herm, a.ws, wb, nullptr); });
}
template <class A, class M> static A with(M m) { A a; m(a); return a; }
#define FWD(stmt) with<Fwd>([&](Fwd& a) { stmt; })
#define BWD(stmt) with<Bwd>([&](Bwd& a) { stmt; })
#define PAIR(stmt) with<Pair>([&](Pair& a) { stmt; })

// every entry of the transform family on one shape under the options in force
static void sweep(const smx_shape& h, bool dropout = true) {
  fwd("p=0", h, Fwd{});
  if (dropout) fwd("p=0.1", h, FWD(a.p = 0.1f));
  fwd("xk=0 bias=0", h, FWD(a.xk = nullptr; a.bias = nullptr));
  for (int ph : {7, 1, 2, 4, 3, 5, 6, 15}) bwd(fmt("phases=%d", ph), h, BWD(a.phases = ph));
  bwd("phases=7 no-w", h, BWD(a.gw_re = a.gw_im = a.gbias = nullptr));
  bwd("phases=1 no-w", h, BWD(a.phases = 1; a.gw_re = a.gw_im = a.gbias = nullptr));
  if (dropout)
    for (int ph : {7, 1, 2}) bwd(fmt("phases=%d p=0.1", ph), h, BWD(a.phases = ph; a.p = 0.1f));
  if (dropout) bwd("phases=7 p=0.1 no-w", h, BWD(a.p = 0.1f; a.gw_re = a.gw_im = a.gbias = nullptr));
  spectrum("", h, Pair{});
  rfft("", h, Pair{});
  rfft("", h, PAIR(a.scale = 0.5f; a.herm = 1));
  irfft("", h, PAIR(a.scale = 0.5f; a.herm = 1));
}

// ---- shapes that reach each plan kind ---------------------------------------------------------------------------------
static const smx_shape DIRECT_1000 = layer(2, 1000, 64, 64), DIRECT_ODD_D = layer(2, 1024, 33, 64),
                       DIRECT_K0 = smx_shape{2, 1024, 64, 64, 1024, 0},
                       D16_SINGLE = layer(8, 400, 64, 200), D16_SPLIT = layer(1, 16000, 2, 256),
                       BANDS1 = layer(8, 1024, 64, 100), BANDS2 = layer(8, 1024, 64, 200), BANDS4 = layer(8, 1024, 64, 512),
                       SPLIT = layer(2, 4096, 64, 256), FOURSTEP = layer(8, 4096, 64, 4096),
                       N2048 = layer(8, 2048, 64, 2048), GROUPS33 = layer(2, 8448, 64, 600),
                       PACKED = layer(128, 1024, 64, 200),                         // 8 Mi elements: the filter is packed
                       PADDED = smx_shape{8, 600, 64, 200, 1024, 200}, NYQUIST_FS = smx_shape{8, 3000, 64, 4096, 4096, 2049};
static const Opts DEFAULT, FS0 = OPT("fourstep=0", o.fourstep = 0),
                  FS0_F80 = OPT("fourstep=0,full8=0", o.fourstep = 0; o.full8 = 0), NSPLIT4 = OPT("nsplit=4", o.nsplit = 4),
                  FORCE_DIRECT = OPT("force_direct=1", o.force_direct = 1), NO_D16 = OPT("decim16=0", o.decim16 = 0);

static void plan_kinds() {
  struct Kind { const char* name; const Opts* o; const smx_shape* h; bool dropout; };
  const Kind kinds[] = {
      {"direct n_fft=1000", &DEFAULT, &DIRECT_1000, true}, {"direct odd D", &DEFAULT, &DIRECT_ODD_D, true},
      {"direct k=0", &DEFAULT, &DIRECT_K0, false},
      {"sixteen-row single", &DEFAULT, &D16_SINGLE, true}, {"sixteen-row split", &DEFAULT, &D16_SPLIT, true},
      {"single launch, 1 band", &DEFAULT, &BANDS1, true}, {"single launch, 2 bands", &DEFAULT, &BANDS2, true},
      {"single launch, 4 bands", &DEFAULT, &BANDS4, true},
      {"residue split by shape", &DEFAULT, &SPLIT, true}, {"residue split by option", &NSPLIT4, &BANDS2, true},
      {"four-step", &DEFAULT, &FOURSTEP, true}, {"four-step at 2048 (the pair: eight bands)", &DEFAULT, &N2048, true},
      {"eight bands", &FS0, &N2048, true},
      {"band groups, 33 tiles", &DEFAULT, &GROUPS33, true}, {"band groups at 2048", &FS0_F80, &N2048, true},
      {"force_direct", &FORCE_DIRECT, &BANDS2, true}, {"decim16=0", &NO_D16, &D16_SINGLE, true},
      {"zero-padded rows", &DEFAULT, &PADDED, false}, {"four-step, padded rows, Nyquist bin", &DEFAULT, &NYQUIST_FS, false},
  };
  for (const Kind& k : kinds) {
    g_last_shape.clear();
    printf("## %s [%s]\n", k.name, k.o->name.c_str());
    Scope sc(*k.o);
    sweep(*k.h, k.dropout);
  }
}

static void variants() {
  g_last_shape.clear(), puts("## filter_pack");
  for (const smx_shape* h : {&BANDS2, &PACKED, &FOURSTEP}) {
    fwd("pack=fill", *h, FWD(a.pack = dp("pack")));
    fwd("pack=ready", *h, FWD(a.pack = dp("pack"); a.conj_w = SMX_FILTER_PACK_READY | 1));
    fwd("ws=0", *h, FWD(a.ws = nullptr));
    bwd("pack=given", *h, BWD(a.pack = dp("pack")));
    bwd("phases=2 pack=given", *h, BWD(a.phases = 2; a.pack = dp("pack")));
  }
  fwd("p=0", PACKED, Fwd{});
  bwd("phases=7", PACKED, Bwd{});
  {
    Scope sc(NSPLIT4);
    fwd("[nsplit=4] pack=fill", PACKED, FWD(a.pack = dp("pack")));
    bwd("[nsplit=4] phases=7", PACKED, Bwd{});
  }
  g_last_shape.clear(), puts("## row_scale");
  for (const smx_shape* h : {&BANDS2, &PADDED, &SPLIT, &FOURSTEP, &NYQUIST_FS}) {
    fwd("row_scale", *h, FWD(a.row_scale = dp("row_scale")));
    for (int ph : {7, 1, 2, 4}) {
      bwd(fmt("phases=%d row_scale", ph), *h, BWD(a.phases = ph; a.row_scale = dp("row_scale")));
      bwd(fmt("phases=%d row_scale grad_row_scale", ph), *h,
          BWD(a.phases = ph; a.row_scale = dp("row_scale"); a.grad_row_scale = dp("grad_row_scale")));
    }
    bwd("row_scale grad_row_scale no-w", *h,
        BWD(a.row_scale = dp("row_scale"); a.grad_row_scale = dp("grad_row_scale"); a.gw_re = a.gw_im = a.gbias = nullptr));
  }
  g_last_shape.clear(), puts("## 2-byte rows");
  for (int io : {0, 1, 2})
    for (const smx_shape* h : {&BANDS1, &BANDS4, &SPLIT, &PACKED, &FOURSTEP, &DIRECT_1000, &D16_SINGLE, &GROUPS33}) {
      if (io == 2 && h != &BANDS4 && h != &SPLIT && h != &FOURSTEP) continue;
      if (io == 0 && h != &BANDS4 && h != &SPLIT && h != &GROUPS33) continue;      // (f32: the f32 entries, seen above)
      fwd(fmt("io=%d", io), *h, FWD(a.io = io));
      bwd(fmt("io=%d", io), *h, BWD(a.io = io));
      if (io && h != &BANDS1 && h != &BANDS4 && h != &SPLIT && h != &PACKED) continue;      // (no native rows: refused)
      fwd(fmt("io=%d p=0.1", io), *h, FWD(a.io = io; a.p = 0.1f));
      for (int ph : {1, 2}) bwd(fmt("io=%d phases=%d", io, ph), *h, BWD(a.io = io; a.phases = ph));
      bwd(fmt("io=%d p=0.1 no-w", io), *h, BWD(a.io = io; a.p = 0.1f; a.gw_re = a.gw_im = a.gbias = nullptr));
    }
  g_last_shape.clear(), puts("## options");
  {
    Scope sc(OPT("fold_gradw=1", o.fold_gradw = 1));
    for (const smx_shape* h : {&BANDS1, &BANDS2, &BANDS4, &SPLIT})
      for (int ph : {7, 15, 3}) bwd(fmt("[fold_gradw=1] phases=%d", ph), *h, BWD(a.phases = ph));
    bwd("[fold_gradw=1] io=1", BANDS2, BWD(a.io = 1));
    bwd("[fold_gradw=1] no-w", BANDS2, BWD(a.gw_re = a.gw_im = a.gbias = nullptr));
  }
  {
    Scope sc(OPT("fs_bgroups=8", o.fs_bgroups = 8));
    for (const smx_shape& h : {layer(16, 2048, 64, 2048), layer(15, 2048, 64, 2048), layer(16, 8192, 64, 8192)})
      for (int ph : {7, 1, 4}) bwd(fmt("[fs_bgroups=8] phases=%d", ph), h, BWD(a.phases = ph));
  }
  for (int v = 0; v <= 4; ++v) {
    const Opts o{fmt("st_plain=%d", v), [v](smx_options& s) { s.st_plain = v; }};
    Scope sc(o);
    for (const smx_shape* h : {&BANDS2, &SPLIT, &FOURSTEP}) {
      fwd("[" + o.name + "]", *h, Fwd{});
      bwd("[" + o.name + "]", *h, Bwd{});
    }
  }
  for (const char* which : {"st_layout_fwd", "st_layout_bwd", "st_layout"})      // (forward and backward launches apart)
    for (int v = -1; v <= 4; ++v) {
      if (which[9] == 0 && v != 2) continue;
      Opts o;
      o.name = fmt("%s=%d", which, v); o.global = which; o.gvalue = v;
      Scope sc(o);
      for (const smx_shape* h : {&BANDS2, &SPLIT}) {
        if (which[10] != 'b') fwd("[" + o.name + "]", *h, Fwd{});
        if (which[10] != 'f') bwd("[" + o.name + "]", *h, Bwd{});
      }
      smx_set_option("st_layout", -2);
    }
  {
    Scope sc(OPT("round=0", o.round = 0));
    for (const smx_shape& h : {layer(640, 1024, 64, 200), SPLIT, FOURSTEP}) {
      fwd("[round=0]", h, Fwd{});
      bwd("[round=0]", h, Bwd{});
    }
  }
  fwd("B=640: rounds", layer(640, 1024, 64, 200), Fwd{});
  bwd("B=640: rounds", layer(640, 1024, 64, 200), Bwd{});
  for (const Opts& o : {OPT("placement=0", o.placement = 0), OPT("placement=1", o.placement = 1)}) {
    Scope sc(o);
    fwd("[" + o.name + "]", BANDS2, Fwd{});
  }
}

// ---- block entries ----------------------------------------------------------------------------------------------------
struct Blk {
  const float *x = dp("x"), *ln_w = dp("ln_w"), *ln_b = dp("ln_b"), *w_re = dp("w_re"), *w_im = dp("w_im"), *bias = dp("bias");
  float *y = dp("y"), *xk = dp("xk"), *stats = dp("ln_stats");
  void* ws = WS;
  long long ws_delta = 0;
  float p = 0.f;
  const void* rng = RNG();
  float* pack = nullptr;
  int io = -1;
  // backward
  const float* g = dp("g");
  float *grad_x = dp("grad_x"), *g_ln_w = dp("g_ln_w"), *g_ln_b = dp("g_ln_b"), *gw_re = dp("gw_re"), *gw_im = dp("gw_im"),
        *gbias = dp("gbias"), *grad_h = dp("grad_h");
  int phases = 7;
};
static void blk_fwd(const std::string& what, const smx_shape& h, const Blk& a) {
  prepare(h.n_fft);
  const size_t wb = ws_bytes(h) + a.ws_delta;
  IN("%s %s %s", a.io >= 0 ? "block_forward_io" : "block_forward_dropout", shp_in(h).c_str(), what.c_str());
  call([&] {
    if (a.io >= 0)
      return smx_block_forward_io(a.x, a.ln_w, a.ln_b, 1e-5f, a.w_re, a.w_im, a.bias, a.y, a.xk, a.stats, a.ws, wb, h.B,
                                  h.n_fft, h.D, h.F, a.p, a.rng, a.pack, nullptr, a.io);
    return smx_block_forward_dropout(a.x, a.ln_w, a.ln_b, 1e-5f, a.w_re, a.w_im, a.bias, a.y, a.xk, a.stats, a.ws, wb, h.B,
                                     h.n_fft, h.D, h.F, a.p, a.rng, a.pack, nullptr);
  });
}
static void blk_bwd(const std::string& what, const smx_shape& h, const Blk& a) {
  prepare(h.n_fft);
  const size_t wb = ws_bytes(h) + a.ws_delta;
  IN("%s %s %s", a.io >= 0 ? "block_backward_io" : "block_backward_dropout", shp_in(h).c_str(), what.c_str());
  call([&] {
    if (a.io >= 0)
      return smx_block_backward_io(a.g, a.x, a.stats, a.ln_w, a.xk, a.w_re, a.w_im, a.grad_x, a.g_ln_w, a.g_ln_b, a.gw_re,
                                   a.gw_im, a.gbias, a.grad_h, a.ws, wb, h.B, h.n_fft, h.D, h.F, a.phases, a.p, a.rng,
                                   a.pack, nullptr, a.io);
    return smx_block_backward_dropout(a.g, a.x, a.stats, a.ln_w, a.xk, a.w_re, a.w_im, a.grad_x, a.g_ln_w, a.g_ln_b,
                                      a.gw_re, a.gw_im, a.gbias, a.ws, wb, h.B, h.n_fft, h.D, h.F, a.phases, a.p, a.rng,
                                      a.pack, nullptr);
  });
}
#define BLK(stmt) with<Blk>([&](Blk& a) { stmt; })
static void blocks() {
  g_last_shape.clear(), puts("## block entries");
  for (const smx_shape* h : {&BANDS2, &PACKED, &SPLIT, &FOURSTEP, &GROUPS33, &D16_SINGLE}) {
    blk_fwd("p=0", *h, Blk{});
    blk_fwd("p=0.1 pack=fill", *h, BLK(a.p = 0.1f; a.pack = dp("pack")));
    for (int ph : {7, 1, 2}) blk_bwd(fmt("phases=%d", ph), *h, BLK(a.phases = ph));
    blk_bwd("p=0.1 pack=given", *h, BLK(a.p = 0.1f; a.pack = dp("pack")));
    for (int io : {0, 1, 2}) {
      if (io != 1 && h != &BANDS2 && h != &SPLIT) continue;
      blk_fwd(fmt("io=%d", io), *h, BLK(a.io = io));
      blk_bwd(fmt("io=%d", io), *h, BLK(a.io = io));
      blk_bwd(fmt("io=%d phases=1", io), *h, BLK(a.io = io; a.phases = 1));
    }
  }
  blk_fwd("io=1: D % 4 != 0", layer(8, 1024, 34, 200), BLK(a.io = 1));
  blk_fwd("D=257", layer(2, 1024, 257, 200), Blk{});
  blk_bwd("D=257", layer(2, 1024, 257, 200), Blk{});
  {
    Scope sc(FS0_F80);
    blk_fwd("[fourstep=0,full8=0]", N2048, Blk{});
    blk_bwd("[fourstep=0,full8=0]", N2048, Blk{});
  }
  {
    Scope sc(FS0);
    blk_fwd("[fourstep=0]", N2048, Blk{});
    blk_bwd("[fourstep=0]", N2048, Blk{});
  }
  g_last_shape.clear(), puts("## block entries: refusals");
  const smx_shape& h = BANDS2;
  blk_fwd("x=0", h, BLK(a.x = nullptr));
  blk_fwd("w_re=0", h, BLK(a.w_re = nullptr));
  blk_fwd("w_im=0", h, BLK(a.w_im = nullptr));
  blk_fwd("y=0", h, BLK(a.y = nullptr));
  blk_fwd("ln_stats=0", h, BLK(a.stats = nullptr));
  blk_fwd("y=x", h, BLK(a.y = (float*)a.x));
  blk_fwd("x+8", h, BLK(a.x = dp("x", 8)));
  blk_fwd("x+4", h, BLK(a.x = dp("x", 4)));
  blk_fwd("ln_w+8", h, BLK(a.ln_w = dp("ln_w", 8)));
  blk_fwd("ln_stats+4", h, BLK(a.stats = dp("ln_stats", 4)));
  blk_fwd("xk+8", h, BLK(a.xk = dp("xk", 8)));
  blk_fwd("io=1 x+4", h, BLK(a.io = 1; a.x = dp("x", 4)));
  blk_fwd("io=1 ln_b+8", h, BLK(a.io = 1; a.ln_b = dp("ln_b", 8)));
  blk_fwd("io=3", h, BLK(a.io = 3));
  blk_fwd("p=1", h, BLK(a.p = 1.f));
  blk_fwd("D=2000", layer(2, 1024, 2000, 200), Blk{});
  blk_fwd("ws=0", h, BLK(a.ws = nullptr));
  blk_fwd("ws=0", SPLIT, BLK(a.ws = nullptr));
  blk_fwd("ws=0", GROUPS33, BLK(a.ws = nullptr));
  blk_fwd("ws short", GROUPS33, BLK(a.ws_delta = -256));
  blk_fwd("ws+128", GROUPS33, BLK(a.ws = (char*)WS + 128));
  blk_bwd("phases=0", h, BLK(a.phases = 0));
  blk_bwd("phases=16", h, BLK(a.phases = 16));
  blk_bwd("x=0", h, BLK(a.x = nullptr));
  blk_bwd("x=0 phases=1", h, BLK(a.x = nullptr; a.phases = 1));
  blk_bwd("grad_x=g", h, BLK(a.grad_x = (float*)a.g));
  blk_bwd("g+8", h, BLK(a.g = dp("g", 8)));
  blk_bwd("ws=0", h, BLK(a.ws = nullptr));
  blk_bwd("D=2000", layer(2, 1024, 2000, 200), Blk{});
  blk_bwd("io=1 grad_h=0", h, BLK(a.io = 1; a.grad_h = nullptr));
  blk_bwd("io=1 grad_h+8", h, BLK(a.io = 1; a.grad_h = dp("grad_h", 8)));
  blk_bwd("io=1 phases=0", h, BLK(a.io = 1; a.phases = 0));
  blk_bwd("io=1 x=0", h, BLK(a.io = 1; a.x = nullptr));
  blk_bwd("io=1 grad_x=x", h, BLK(a.io = 1; a.grad_x = (float*)a.x));
  blk_bwd("io=1 g+4", h, BLK(a.io = 1; a.g = dp("g", 4)));
  blk_bwd("io=1 ln_w+8", h, BLK(a.io = 1; a.ln_w = dp("ln_w", 8)));
  blk_bwd("io=3", h, BLK(a.io = 3));
  blk_bwd("io=1 ws=0", h, BLK(a.io = 1; a.ws = nullptr));
}

// ---- convolution ------------------------------------------------------------------------------------------------------
struct Conv {
  const float *x = dp("x"), *h_re = dp("h_re"), *h_im = dp("h_im"), *row_scale = dp("row_scale");
  float *y = dp("y"), *xs = dp("x_spectra");
  void* ws = WS;
  long long ws_delta = 0;
  int io = -1;
  float *gh_re = dp("grad_h_re"), *gh_im = dp("grad_h_im"), *grs = dp("grad_row_scale");
};
static size_t conv_bytes(const smx_shape& h) {
  size_t n = 0, save = 0;
  return smx_conv_workspace_bytes(&h, &n, &save) ? 4096 : n;
}
static void conv_fwd(const std::string& what, const smx_shape& h, const Conv& a) {
  prepare(h.n_fft);
  const size_t wb = conv_bytes(h) + a.ws_delta;
  IN("%s %s %s", a.io >= 0 ? "conv_forward_io" : "conv_forward", shp_in(h).c_str(), what.c_str());
  call([&] {
    if (a.io >= 0) return smx_conv_forward_io(&h, a.x, a.h_re, a.h_im, a.row_scale, a.y, a.xs, a.ws, wb, a.io, nullptr);
    return smx_conv_forward(&h, a.x, a.h_re, a.h_im, a.row_scale, a.y, a.xs, a.ws, wb, nullptr);
  });
}
static void conv_bwd(const std::string& what, const smx_shape& h, const Conv& a) {
  prepare(h.n_fft);
  const size_t wb = conv_bytes(h) + a.ws_delta;
  IN("%s %s %s", a.io >= 0 ? "conv_backward_io" : "conv_backward", shp_in(h).c_str(), what.c_str());
  call([&] {
    if (a.io >= 0)
      return smx_conv_backward_io(&h, a.x, a.xs, a.h_re, a.h_im, a.row_scale, a.y, a.gh_re, a.gh_im, a.grs, a.ws, wb, a.io,
                                  nullptr);
    return smx_conv_backward(&h, a.x, a.xs, a.h_re, a.h_im, a.row_scale, a.y, a.gh_re, a.gh_im, a.grs, a.ws, wb, nullptr);
  });
}
#define CONV(stmt) with<Conv>([&](Conv& a) { stmt; })
static smx_shape conv_shape(int B, int rows, int D, int n_fft) { return smx_shape{B, rows, D, 0, n_fft, 0}; }
static void convolution() {
  g_last_shape.clear(), puts("## convolution");
  const smx_shape small = conv_shape(8, 1024, 64, 2048), mid = conv_shape(32, 1024, 64, 2048),
                  big = conv_shape(512, 200, 64, 512), longer = conv_shape(2, 5000, 64, 8192), ragged = conv_shape(3, 700, 34, 1024);
  for (int c1 = 0; c1 <= 3; ++c1) {
    const Opts o{fmt("conv1=%d", c1), [c1](smx_options& s) { s.conv1 = c1; }};
    Scope sc(o);
    for (const smx_shape* h : {&small, &mid, &big, &longer, &ragged}) {
      if (c1 != 1 && (h == &longer || h == &ragged || (h == &big && c1 != 2))) continue;
      conv_fwd("[" + o.name + "]", *h, Conv{});
      conv_bwd("[" + o.name + "]", *h, Conv{});
      if (c1 == 1 || h == &small)
        for (int io : {0, 1, 2}) {
          conv_fwd("[" + o.name + "]" + fmt(" io=%d", io), *h, CONV(a.io = io));
          conv_bwd("[" + o.name + "]" + fmt(" io=%d", io), *h, CONV(a.io = io));
        }
    }
  }
  for (const smx_shape* h : {&small, &mid}) {
    conv_fwd("x_spectra=0 row_scale=0", *h, CONV(a.xs = nullptr; a.row_scale = nullptr));
    conv_bwd("no gradients of h and row_scale", *h, CONV(a.gh_re = a.gh_im = a.grs = nullptr; a.row_scale = nullptr));
  }
  g_last_shape.clear(), puts("## convolution: refusals");
  for (const smx_shape* h : {&small, &mid}) {
    conv_fwd("ws=0", *h, CONV(a.ws = nullptr));
    conv_fwd("ws short", *h, CONV(a.ws_delta = -1));
    conv_fwd("ws+128", *h, CONV(a.ws = (char*)WS + 128));
    conv_bwd("ws=0", *h, CONV(a.ws = nullptr));
    conv_bwd("ws short", *h, CONV(a.ws_delta = -1));
    conv_bwd("ws+128", *h, CONV(a.ws = (char*)WS + 128));
  }
  conv_fwd("x=0", mid, CONV(a.x = nullptr));
  conv_fwd("y=0", mid, CONV(a.y = nullptr));
  conv_fwd("h_re=0", mid, CONV(a.h_re = nullptr));
  conv_fwd("h_im=0", mid, CONV(a.h_im = nullptr));
  conv_fwd("x+4", mid, CONV(a.x = dp("x", 4)));
  conv_fwd("x_spectra+4", mid, CONV(a.xs = dp("x_spectra", 4)));
  conv_fwd("io=1 x+2", mid, CONV(a.io = 1; a.x = dp("x", 2)));
  conv_fwd("io=1 x_spectra+4", mid, CONV(a.io = 1; a.xs = dp("x_spectra", 4)));
  conv_fwd("io=3", mid, CONV(a.io = 3));
  conv_fwd("n_fft=768", conv_shape(8, 700, 64, 768), Conv{});
  conv_fwd("odd D", conv_shape(8, 700, 33, 1024), Conv{});
  conv_fwd("rows > n_fft", conv_shape(8, 2000, 64, 1024), Conv{});
  conv_bwd("g=0", mid, CONV(a.x = nullptr));
  conv_bwd("x_spectra=0", mid, CONV(a.xs = nullptr));
  conv_bwd("grad_x=0", mid, CONV(a.y = nullptr));
  conv_bwd("grad_h_im=0", mid, CONV(a.gh_im = nullptr));
  conv_bwd("g+4", mid, CONV(a.x = dp("x", 4)));
  conv_bwd("io=1 g+2", mid, CONV(a.io = 1; a.x = dp("x", 2)));
  conv_bwd("io=1 x_spectra+4", mid, CONV(a.io = 1; a.xs = dp("x_spectra", 4)));
  conv_bwd("h_re=0", mid, CONV(a.h_re = nullptr));
  conv_bwd("io=3", mid, CONV(a.io = 3));
  conv_bwd("n_fft=768", conv_shape(8, 700, 64, 768), Conv{});

  g_last_shape.clear(), puts("## cfft, phase filter, response");
  auto cfft = [](const std::string& what, const smx_shape& h, const float* z, float* out, void* ws, long long delta) {
    prepare(h.n_fft);
    size_t wb = 0;
    if (smx_cfft_workspace_bytes(&h, &wb)) wb = 1 << 20;
    IN("cfft_ex %s %s", shp_in(h).c_str(), what.c_str());
    call([&] { return smx_cfft_ex(&h, z, out, ws, wb + delta, nullptr); });
  };
  for (const smx_shape& h : {conv_shape(8, 1024, 64, 1024), conv_shape(2, 500, 34, 512), conv_shape(1, 9216, 64, 9216),
                             conv_shape(64, 4096, 256, 4096)})
    cfft("", h, dp("x"), dp("y"), WS, 0);
  const smx_shape c4 = conv_shape(8, 1024, 64, 1024);
  cfft("n_fft=768", conv_shape(8, 768, 64, 768), dp("x"), dp("y"), WS, 0);
  cfft("odd D", conv_shape(8, 1024, 33, 1024), dp("x"), dp("y"), WS, 0);
  cfft("z=0", c4, nullptr, dp("y"), WS, 0);
  cfft("out=0", c4, dp("x"), nullptr, WS, 0);
  cfft("z+4", c4, dp("x", 4), dp("y"), WS, 0);
  cfft("ws=0", c4, dp("x"), dp("y"), nullptr, 0);
  cfft("ws short", c4, dp("x"), dp("y"), WS, -1);
  cfft("ws+128", c4, dp("x"), dp("y"), (char*)WS + 128, 0);
  IN("cfft_ex shape=0");
  call([&] { return smx_cfft_ex(nullptr, dp("x"), dp("y"), WS, 1 << 20, nullptr); });

  IN("phase_filter D=64 k=200 n_fft=1024");
  call([&] { return smx_phase_filter(dp("magnitude"), dp("phase"), 64, 200, 1024, dp("w_re"), dp("w_im"), nullptr); });
  IN("phase_filter k > n_fft/2+1");
  call([&] { return smx_phase_filter(dp("magnitude"), dp("phase"), 64, 600, 1024, dp("w_re"), dp("w_im"), nullptr); });
  IN("phase_filter phase=0");
  call([&] { return smx_phase_filter(dp("magnitude"), nullptr, 64, 200, 1024, dp("w_re"), dp("w_im"), nullptr); });
  IN("phase_filter_backward D=64 k=200 n_fft=1024 pitch=256");
  call([&] { return smx_phase_filter_backward(dp("magnitude"), dp("phase"), dp("gw_re"), dp("gw_im"), 64, 200, 1024, 256,
                                              dp("g_m"), dp("g_p"), nullptr); });
  IN("phase_filter_backward pitch < k");
  call([&] { return smx_phase_filter_backward(dp("magnitude"), dp("phase"), dp("gw_re"), dp("gw_im"), 64, 200, 1024, 100,
                                              dp("g_m"), dp("g_p"), nullptr); });
  IN("phase_filter_backward grad_w_re=0");
  call([&] { return smx_phase_filter_backward(dp("magnitude"), dp("phase"), nullptr, dp("gw_im"), 64, 200, 1024, 256,
                                              dp("g_m"), dp("g_p"), nullptr); });
  prepare(2048);
  IN("conv_response n_fft=2048 taps=128");
  call([&] { return smx_conv_response(2048, 128, dp("kernel"), dp("logits"), dp("mask"), dp("h_re"), dp("h_im"), nullptr); });
  IN("conv_response taps > n_fft");
  call([&] { return smx_conv_response(2048, 4096, dp("kernel"), dp("logits"), dp("mask"), dp("h_re"), dp("h_im"), nullptr); });
  IN("conv_response kernel=0");
  call([&] { return smx_conv_response(2048, 128, nullptr, dp("logits"), dp("mask"), dp("h_re"), dp("h_im"), nullptr); });
  IN("conv_response_backward n_fft=2048 taps=128 n_logits=1025");
  call([&] { return smx_conv_response_backward(2048, 128, 1025, dp("kernel"), dp("logits"), dp("mask"), dp("grad_h_re"),
                                               dp("grad_h_im"), dp("grad_kernel"), dp("grad_logits"), nullptr); });
  IN("conv_response_backward n_logits=100");
  call([&] { return smx_conv_response_backward(2048, 128, 100, dp("kernel"), dp("logits"), dp("mask"), dp("grad_h_re"),
                                               dp("grad_h_im"), dp("grad_kernel"), dp("grad_logits"), nullptr); });
  IN("conv_response_backward grad_h_re=0");
  call([&] { return smx_conv_response_backward(2048, 128, 1025, dp("kernel"), dp("logits"), dp("mask"), nullptr,
                                               dp("grad_h_im"), dp("grad_kernel"), dp("grad_logits"), nullptr); });
}

// ---- the smaller ops: one accepted call each (more where an input selects a kernel), and the workspace refusals ----
// f(ws, bytes): the op with dummy tensors; need: its workspace query
static void with_ws(const char* name, size_t need, const std::function<int(void*, size_t)>& f) {
  struct Case { const char* what; void* ws; long long delta; };
  for (const Case& c : {Case{"", WS, 0}, Case{"ws=0", nullptr, 0}, Case{"ws short", WS, -1}, Case{"ws+128", (char*)WS + 128, 0}}) {
    IN("%s %s", name, c.what);
    call([&] { return f(c.ws, need + c.delta); });
  }
}
static void small_ops() {
  g_last_shape.clear(), puts("## smaller ops");
  size_t need = 0;
  float *A = dp("a"), *B_ = dp("b"), *C = dp("c"), *E = dp("e"), *G = dp("g"), *X = dp("x"), *Y = dp("y"), *W = dp("w");
  IN("dwconv3_workspace_bytes (4,100,96)");
  call([&] { const int rc = smx_dwconv3_workspace_bytes(4, 100, 96, &need); g_rec = fmt("%zu", need); return rc; });
  IN("dwconv3_forward (4,100,96)");
  call([&] { return smx_dwconv3_forward(X, W, dp("bias"), dp("scale"), Y, 4, 100, 96, nullptr); });
  smx_dwconv3_workspace_bytes(4, 100, 96, &need);
  with_ws("dwconv3_backward (4,100,96)", need, [&](void* ws, size_t n) {
    return smx_dwconv3_backward(G, X, W, dp("bias"), dp("scale"), dp("grad_x"), dp("grad_w"), dp("gbias"), dp("grad_scale"), ws, n,
                                4, 100, 96, nullptr);
  });
  for (int planar = 0; planar < 2; ++planar) {
    IN("spectral_ln_forward (4,65,96) planar=%d", planar);
    call([&] { return smx_spectral_ln_forward(X, dp("gamma"), dp("beta"), 1e-5f, Y, planar, 4, 65, 96, nullptr); });
    IN("spectral_ln_backward (4,65,96) planar=%d", planar);
    call([&] { return smx_spectral_ln_backward(G, X, dp("gamma"), dp("beta"), 1e-5f, dp("grad_x"), dp("g_gamma"), dp("g_beta"),
                                               planar, 4, 65, 96, nullptr); });
  }
  IN("planar_cmul_forward (4,65,96)");
  call([&] { return smx_planar_cmul_forward(X, A, B_, Y, 4, 65, 96, nullptr); });
  IN("planar_cmul_backward (4,65,96)");
  call([&] { return smx_planar_cmul_backward(G, X, A, B_, dp("grad_x"), dp("ga"), dp("gb"), 4, 65, 96, nullptr); });
  IN("planar_add n=24960");
  call([&] { return smx_planar_add(A, X, Y, 24960, nullptr); });
  IN("planar_split n=24960");
  call([&] { return smx_planar_split(G, Y, 24960, nullptr); });

  IN("spectral_gate_workspace_bytes (4,65,96)");
  call([&] { const int rc = smx_spectral_gate_workspace_bytes(4, 65, 96, &need); g_rec = fmt("%zu", need); return rc; });
  IN("spectral_gate_forward (4,65,96)");
  call([&] { return smx_spectral_gate_forward(X, A, dp("u"), dp("p"), dp("q"), dp("m"), Y, 4, 65, 96, nullptr); });
  with_ws("spectral_gate_backward (4,65,96)", need, [&](void* ws, size_t n) {
    return smx_spectral_gate_backward(G, X, A, dp("u"), dp("p"), dp("q"), dp("m"), dp("grad_x"), dp("s1"), dp("rc"), dp("rp"), ws, n,
                                      4, 65, 96, nullptr);
  });
  IN("mix_workspace_bytes");
  call([&] { const int rc = smx_mix_workspace_bytes(&need); g_rec = fmt("%zu", need); return rc; });
  IN("mix_forward n=24960");
  call([&] { return smx_mix_forward(X, A, B_, C, W, 0.1f, Y, 24960, nullptr); });
  with_ws("mix_backward n=24960", need, [&](void* ws, size_t n) {
    return smx_mix_backward(G, A, B_, W, 0.1f, dp("ga"), dp("gb"), dp("gc"), dp("grad_w"), ws, n, 24960, nullptr);
  });

  IN("enh_workspace_bytes (4,100,96)");
  call([&] { const int rc = smx_enh_workspace_bytes(4, 100, 96, &need); g_rec = fmt("%zu", need); return rc; });
  for (int norm = 0; norm < 2; ++norm)
    for (float p : {0.f, 0.1f}) {
      IN("rope_norm_forward (4,100,96) norm=%d p=%g", norm, (double)p);
      call([&] { return smx_rope_norm_forward(X, dp("rotation"), 128, A, B_, C, E, 1e-5f, 1e-5f, dp("x1"), dp("h2"), dp("stats"), 4,
                                              100, 96, norm, p, RNG(), nullptr); });
      IN("rope_norm_backward (4,100,96) norm=%d p=%g", norm, (double)p);
      call([&] { return smx_rope_norm_backward(G, dp("gh2"), X, dp("rotation"), 128, A, B_, C, dp("stats"), dp("grad_x"), dp("ga"),
                                               dp("gb"), dp("gc"), dp("ge"), WS, need, 4, 100, 96, norm, p, RNG(), nullptr); });
    }
  with_ws("rope_norm_backward (4,100,96) norm=1", need, [&](void* ws, size_t n) {
    return smx_rope_norm_backward(G, dp("gh2"), X, dp("rotation"), 128, A, B_, C, dp("stats"), dp("grad_x"), dp("ga"), dp("gb"),
                                  dp("gc"), dp("ge"), ws, n, 4, 100, 96, 1, 0.f, RNG(), nullptr);
  });
  for (float p : {0.f, 0.1f}) {
    IN("residual_norm_forward (4,100,96) p=%g", (double)p);
    call([&] { return smx_residual_norm_forward(dp("x1"), dp("p"), A, B_, 1e-5f, dp("x2"), dp("h3"), dp("stats"), 4, 100, 96, p, RNG(),
                                                nullptr); });
    IN("gate_blend_forward (4,100,96) p=%g", (double)p);
    call([&] { return smx_gate_blend_forward(A, dp("v"), dp("x2"), C, E, 1e-5f, dp("x3"), dp("stats"), 4, 100, 96, p, RNG(), nullptr); });
  }
  with_ws("residual_norm_backward (4,100,96)", need, [&](void* ws, size_t n) {
    return smx_residual_norm_backward(G, dp("gh3"), dp("x2"), A, dp("stats"), dp("grad_x1"), dp("grad_p"), dp("ga"), dp("gb"), ws, n, 4,
                                      100, 96, 0.1f, RNG(), nullptr);
  });
  with_ws("gate_blend_backward (4,100,96)", need, [&](void* ws, size_t n) {
    return smx_gate_blend_backward(G, A, dp("v"), C, E, dp("stats"), dp("ga"), dp("gv"), dp("gc"), dp("ge"), ws, n, 4, 100, 96, 0.1f,
                                   RNG(), nullptr);
  });

  IN("ema_workspace_bytes (4,12,33)");
  call([&] { const int rc = smx_ema_workspace_bytes(4, 12, 33, &need); g_rec = fmt("%zu", need); return rc; });
  for (int mode : {0, 1, 2}) {
    IN("ema_scan_forward (4,12,33) mode=%d", mode);
    call([&] { return smx_ema_scan_forward(X, dp("init"), dp("rho"), dp("theta"), Y, mode, 4, 12, 33, nullptr); });
    IN("ema_tokens_forward (4,768,L64) mode=%d", mode);
    call([&] { return smx_ema_tokens_forward(dp("tokens"), 1, 800, dp("init"), dp("rho"), dp("theta"), Y, mode, 4, 768, 64, nullptr); });
  }
  with_ws("ema_scan_backward (4,12,33)", need, [&](void* ws, size_t n) {
    return smx_ema_scan_backward(G, X, dp("init"), dp("rho"), dp("theta"), dp("grad_x"), dp("grad_init"), dp("grad_rho"),
                                 dp("grad_theta"), ws, n, 0, 4, 12, 33, nullptr);
  });
  with_ws("ema_tokens_backward (4,768,L64)", need, [&](void* ws, size_t n) {
    return smx_ema_tokens_backward(G, dp("tokens"), 8, 800, dp("init"), dp("rho"), dp("theta"), dp("grad_init"), dp("grad_rho"),
                                   dp("grad_theta"), ws, n, 1, 4, 768, 64, nullptr);
  });

  IN("stream_push (Bt 3, T 256, C 96, chunk 16)");
  call([&] { return smx_stream_push(X, A, B_, 1e-5f, dp("ring"), dp("sum"), dp<int>("pos"), dp("pooled"), 3, 256, 96, 16, nullptr); });
  IN("stream_conv (Bt 3, T 256, K 128, C 96, chunk 16)");
  call([&] { return smx_stream_conv(X, dp("ring"), dp<int>("pos"), dp("taps"), dp("scale"), A, B_, 1e-5f, Y, dp("ff_in"), 3, 256,
                                    128, 96, 16, nullptr); });

  IN("grad_w (8,1024,64,F200)");
  call([&] { return smx_grad_w(dp("xk"), dp("gk"), dp("gw_re"), dp("gw_im"), dp("gbias"), 8, 1024, 64, 200, nullptr); });
  for (int conj = 0; conj < 2; ++conj) {
    IN("wfilter_forward (8,1024,64,F200) conj_w=%d", conj);
    call([&] { return smx_wfilter_forward(X, dp("w_re"), dp("w_im"), Y, 8, 1024, 64, 200, conj, nullptr); });
    IN("cmul batch=8 inner=65536 conj_w=%d", conj);
    call([&] { return smx_cmul(X, W, Y, 8, 65536, conj, nullptr); });
  }
  IN("wfilter_grad_w (8,1024,64,F200)");
  call([&] { return smx_wfilter_grad_w(X, G, dp("gw_re"), dp("gw_im"), 8, 1024, 64, 200, nullptr); });
  IN("cmul inner=0");
  call([&] { return smx_cmul(X, W, Y, 8, 0, 0, nullptr); });
  IN("cmul_grad_w batch=8 inner=65536");
  call([&] { return smx_cmul_grad_w(X, G, dp("grad_w"), 8, 65536, nullptr); });
  IN("rng_next");
  call([&] { return smx_rng_next((void*)RNG(), dp("saved"), nullptr); });
}

// ---- refusals of the transform entries, one fault at a time ---------------------------------------------------------------
// ("fused dropout is not available with zero-padded rows" has no case: no entry takes both a dropout probability and
// rows < n_fft)
static void refusals() {
  g_last_shape.clear(), puts("## refusals: forward");
  for (const smx_shape* h : {&D16_SPLIT, &SPLIT, &FOURSTEP, &GROUPS33, &DIRECT_1000}) {
    fwd("ws=0", *h, FWD(a.ws = nullptr));
    fwd("ws short", *h, FWD(a.ws_delta = -1));
    fwd("ws+128", *h, FWD(a.ws = (char*)WS + 128));
  }
  fwd("ws short", BANDS2, FWD(a.ws_delta = -1));            // (accepted: the single launch needs none)
  fwd("ws+128", BANDS2, FWD(a.ws = (char*)WS + 128));
  fwd("io=1 ws=0", SPLIT, FWD(a.io = 1; a.ws = nullptr));
  {
    Scope sc(FS0);
    fwd("[fourstep=0] ws=0", N2048, FWD(a.ws = nullptr));
  }
  const smx_shape& h = BANDS2;
  fwd("x=0", h, FWD(a.x = nullptr));
  fwd("w_re=0", h, FWD(a.w_re = nullptr));
  fwd("w_im=0", h, FWD(a.w_im = nullptr));
  fwd("y=0", h, FWD(a.y = nullptr));
  fwd("x+4", h, FWD(a.x = dp("x", 4)));
  fwd("y+4", h, FWD(a.y = dp("y", 4)));
  fwd("xk+8", h, FWD(a.xk = dp("xk", 8)));
  fwd("pack+8", h, FWD(a.pack = dp("pack", 8)));
  fwd("pack ready without pack", h, FWD(a.conj_w = SMX_FILTER_PACK_READY));
  fwd("p=1", h, FWD(a.p = 1.f));
  fwd("p=-0.5", h, FWD(a.p = -0.5f));
  fwd("p=0.1 rng=0", h, FWD(a.p = 0.1f; a.rng = nullptr));
  fwd("p=0.1 rng+4", h, FWD(a.p = 0.1f; a.rng = dp("rng", 4)));
  fwd("io=1 x+2", h, FWD(a.io = 1; a.x = dp("x", 2)));
  fwd("io=1 x+4", h, FWD(a.io = 1; a.x = dp("x", 4)));
  fwd("io=3", h, FWD(a.io = 3));
  fwd("B=0", layer(0, 1024, 64, 200), Fwd{});
  fwd("y=x", GROUPS33, FWD(a.y = (float*)a.x));
  fwd("y=x", FOURSTEP, FWD(a.y = (float*)a.x));
  fwd("row_scale", GROUPS33, FWD(a.row_scale = dp("row_scale")));
  fwd("row_scale", DIRECT_1000, FWD(a.row_scale = dp("row_scale")));
  fwd("row_scale", D16_SINGLE, FWD(a.row_scale = dp("row_scale")));
  {
    Scope sc(FS0);
    fwd("[fourstep=0] row_scale", N2048, FWD(a.row_scale = dp("row_scale")));
  }
  IN("forward_ex shape=0");
  call([&] { return smx_forward_ex(nullptr, dp("x"), dp("w_re"), dp("w_im"), nullptr, dp("y"), nullptr, WS, 1 << 20, 0, nullptr, nullptr, nullptr); });
  fwd("rows > n_fft", smx_shape{8, 2000, 64, 200, 1024, 200}, Fwd{});
  fwd("k > F", smx_shape{8, 1024, 64, 100, 1024, 200}, Fwd{});

  g_last_shape.clear(), puts("## refusals: backward");
  for (const smx_shape* hh : {&D16_SINGLE, &BANDS2, &SPLIT, &FOURSTEP, &GROUPS33, &DIRECT_1000}) {
    bwd("ws=0", *hh, BWD(a.ws = nullptr));
    bwd("ws short", *hh, BWD(a.ws_delta = -1));
    bwd("ws+128", *hh, BWD(a.ws = (char*)WS + 128));
  }
  bwd("g=0", h, BWD(a.g = nullptr));
  bwd("w_re=0", h, BWD(a.w_re = nullptr));
  bwd("w_im=0", h, BWD(a.w_im = nullptr));
  bwd("grad_x=0", h, BWD(a.grad_x = nullptr));
  bwd("grad_x=0 phases=5", h, BWD(a.grad_x = nullptr; a.phases = 5));
  bwd("gw_im=0", h, BWD(a.gw_im = nullptr));
  bwd("gbias=0", h, BWD(a.gbias = nullptr));
  bwd("g+4", h, BWD(a.g = dp("g", 4)));
  bwd("grad_x+4", h, BWD(a.grad_x = dp("grad_x", 4)));
  bwd("xk+8", h, BWD(a.xk = dp("xk", 8)));
  bwd("xk=0", h, BWD(a.xk = nullptr));
  bwd("xk=0 no-w", h, BWD(a.xk = nullptr; a.gw_re = a.gw_im = a.gbias = nullptr));
  bwd("xk=0 no-w p=0.1", h, BWD(a.xk = nullptr; a.p = 0.1f; a.gw_re = a.gw_im = a.gbias = nullptr));
  bwd("pack+8", h, BWD(a.pack = dp("pack", 8)));
  bwd("phases=0", h, BWD(a.phases = 0));
  bwd("phases=8", h, BWD(a.phases = 8));
  bwd("phases=16", h, BWD(a.phases = 16));
  bwd("p=1", h, BWD(a.p = 1.f));
  bwd("p=0.1 rng=0", h, BWD(a.p = 0.1f; a.rng = nullptr));
  bwd("io=1 g+2", h, BWD(a.io = 1; a.g = dp("g", 2)));
  bwd("io=1 grad_x+4", h, BWD(a.io = 1; a.grad_x = dp("grad_x", 4)));
  bwd("io=3", h, BWD(a.io = 3));
  bwd("grad_row_scale without row_scale", h, BWD(a.grad_row_scale = dp("grad_row_scale")));
  bwd("row_scale", GROUPS33, BWD(a.row_scale = dp("row_scale")));
  bwd("row_scale", DIRECT_1000, BWD(a.row_scale = dp("row_scale")));
  bwd("row_scale", D16_SINGLE, BWD(a.row_scale = dp("row_scale")));
  bwd("p=0.1 grad_x=0 phases=1", FOURSTEP, BWD(a.p = 0.1f; a.grad_x = nullptr; a.phases = 1));
  bwd("p=0.1 grad_x=0 phases=1", DIRECT_1000, BWD(a.p = 0.1f; a.grad_x = nullptr; a.phases = 1));
  {
    Scope sc(FS0);
    bwd("[fourstep=0] p=0.1 phases=1", N2048, BWD(a.p = 0.1f; a.phases = 1));
    bwd("[fourstep=0] p=0.1 phases=3", N2048, BWD(a.p = 0.1f; a.phases = 3));
    bwd("[fourstep=0] row_scale", N2048, BWD(a.row_scale = dp("row_scale")));
  }
  IN("backward_ex shape=0");
  call([&] { return smx_backward_ex(nullptr, dp("g"), dp("xk"), dp("w_re"), dp("w_im"), dp("grad_x"), nullptr, nullptr, nullptr, WS,
                                    1 << 20, 7, nullptr, nullptr, nullptr, nullptr); });

  g_last_shape.clear(), puts("## refusals: spectrum, rfft, irfft");
  for (const smx_shape* hh : {&D16_SPLIT, &SPLIT, &FOURSTEP, &N2048, &GROUPS33}) {
    spectrum("ws=0", *hh, PAIR(a.ws = nullptr));
    spectrum("ws short", *hh, PAIR(a.ws_delta = -1));
    spectrum("ws+128", *hh, PAIR(a.ws = (char*)WS + 128));
    rfft("ws=0", *hh, PAIR(a.ws = nullptr));
    irfft("ws=0", *hh, PAIR(a.ws = nullptr));
    irfft("ws short", *hh, PAIR(a.ws_delta = -1));
    irfft("ws+128", *hh, PAIR(a.ws = (char*)WS + 128));
  }
  spectrum("ws=0", BANDS2, PAIR(a.ws = nullptr));           // (accepted)
  irfft("ws=0", BANDS2, PAIR(a.ws = nullptr));
  irfft("ws=0", DIRECT_1000, PAIR(a.ws = nullptr));
  spectrum("x=0", h, PAIR(a.x = nullptr));
  spectrum("xk=0", h, PAIR(a.spec = nullptr));
  spectrum("x+4", h, PAIR(a.x = dp("x", 4)));
  spectrum("xk+8", h, PAIR(a.spec = dp("xk", 8)));
  rfft("x=0", h, PAIR(a.x = nullptr));
  rfft("x=0", N2048, PAIR(a.x = nullptr));
  rfft("x+4", N2048, PAIR(a.x = dp("x", 4)));
  rfft("spec+8", N2048, PAIR(a.spec = dp("xk", 8)));
  irfft("y=0", h, PAIR(a.y = nullptr));
  irfft("spec=0", h, PAIR(a.spec = nullptr));
  irfft("y+4", h, PAIR(a.y = dp("y", 4)));
  irfft("spec+8", h, PAIR(a.spec = dp("xk", 8)));
  irfft("k=0 y=0", DIRECT_K0, PAIR(a.y = nullptr));

  g_last_shape.clear(), puts("## refusals: stream capture with the tables absent");
  g_capturing = true;
  const smx_shape fresh = layer(8, 1536, 64, 200), fresh_groups = layer(2, 8704, 64, 1100);
  IN("forward_dropout %s capturing", shp(fresh).c_str());
  call([&] { return smx_forward_dropout(dp("x"), dp("w_re"), dp("w_im"), nullptr, dp("y"), nullptr, WS, ws_bytes(fresh), 8, 1536, 64,
                                        200, 0, 0.f, nullptr, nullptr, nullptr); });
  IN("conv_response n_fft=1536 capturing");
  call([&] { return smx_conv_response(1536, 128, dp("kernel"), nullptr, nullptr, dp("h_re"), dp("h_im"), nullptr); });
  g_capturing = false;
  prepare(8704);
  g_capturing = true;                                       // the tables of n_fft are there, the band groups' are not
  IN("forward_dropout %s capturing", shp(fresh_groups).c_str());
  call([&] { return smx_forward_dropout(dp("x"), dp("w_re"), dp("w_im"), nullptr, dp("y"), nullptr, WS, ws_bytes(fresh_groups), 2,
                                        8704, 64, 1100, 0, 0.f, nullptr, nullptr, nullptr); });
  IN("forward_dropout %s capturing, tables present", shp(BANDS2).c_str());
  call([&] { return smx_forward_dropout(dp("x"), dp("w_re"), dp("w_im"), nullptr, dp("y"), nullptr, WS, ws_bytes(BANDS2), 8, 1024, 64,
                                        200, 0, 0.f, nullptr, nullptr, nullptr); });
  g_capturing = false;
}

// ---- the newer ops: every branch of an entry or launcher that selects an instance, a grid or an argument; every refusal --
// (nothing is read or written here, so a size costs nothing: the shapes are the ones that reach the branches)
static void answer(const std::string& v) { call([&] { g_rec = v; return 0; }); }
static void query(const std::function<int(size_t*)>& f) {
  call([&] { size_t n = 0; const int rc = f(&n); if (!rc) g_rec = fmt("%zu", n); return rc; });
}
static size_t sized(const std::function<int(size_t*)>& f) { size_t n = 0; return f(&n) ? 4096 : n; }

static void word_targets_and_head() {
  void* TK = dp<char>("tokens");
  float *PH = dp("phase"), *BD = dp("boundary");
  auto wt = [&](const char* what, const void* tokens, int tb, long long stride, float* phase, float* boundary, int B, int T) {
    IN("word_targets (%d,%d) token_bytes=%d stride=%lld %s", B, T, tb, stride, what);
    call([&] { return smx_word_targets(tokens, tb, stride, phase, boundary, B, T, nullptr); });
  };
  for (int tb : {1, 8}) {
    wt("phase", TK, tb, 128, PH, nullptr, 3, 100);
    wt("boundary", TK, tb, 128, nullptr, BD, 3, 100);
    wt("both", TK, tb, 128, PH, BD, 3, 100);
  }
  wt("T=65536", TK, 1, 65536, PH, BD, 2, 65536);
  wt("B=0", TK, 1, 128, PH, BD, 0, 100);
  wt("T=65537", TK, 1, 70000, PH, BD, 3, 65537);
  wt("B*T=2^31", TK, 1, 65536, PH, BD, 32768, 65536);
  wt("token_bytes=4", TK, 4, 128, PH, BD, 3, 100);
  wt("tokens=0", nullptr, 1, 128, PH, BD, 3, 100);
  wt("both outputs NULL", TK, 1, 128, nullptr, nullptr, 3, 100);
  wt("row_stride < T", TK, 1, 99, PH, BD, 3, 100);
  wt("tokens+4", dp<char>("tokens", 4), 8, 128, PH, BD, 3, 100);
  wt("tokens+4", dp<char>("tokens", 4), 1, 128, PH, BD, 3, 100);        // (accepted: bytes)
  wt("phase+4", TK, 1, 128, dp("phase", 4), BD, 3, 100);
  wt("boundary+2", TK, 1, 128, PH, dp("boundary", 2), 3, 100);

  float *H = dp("h"), *W = dp("w"), *Bv = dp("b"), *Y = dp("y"), *G = dp("g");
  IN("head_supported C=96,97,1000,1024,1025,1028,4096,4100,0 x O=0..3");
  {
    std::string v;
    for (int C : {96, 97, 1000, 1024, 1025, 1028, 4096, 4100, 0}) {
      for (int O = 0; O <= 3; ++O) v += fmt("%d", smx_head_supported(C, O));
      v += " ";
    }
    answer(v);
  }
  auto head_ws = [&](const char* what, long long R, int C, int O, bool out = true) {
    IN("head_workspace_bytes (%lld,%d) O=%d %s", R, C, O, what);
    query([&](size_t* n) { return smx_head_workspace_bytes(R, C, O, out ? n : nullptr); });
  };
  head_ws("", 37, 96, 1);
  head_ws("", 37, 96, 2);
  head_ws("", 100000, 96, 2);
  head_ws("out=0", 37, 96, 1, false);
  head_ws("R=0", 0, 96, 1);
  head_ws("O=3", 37, 96, 3);
  head_ws("C=1025", 37, 1025, 1);
  head_ws("R*C=2^40", 1ll << 28, 4096, 1);
  auto head_fwd = [&](const char* what, const float* h, const float* w, const float* b, float* y, long long R, int C, int O) {
    IN("head_forward (%lld,%d) O=%d %s", R, C, O, what);
    call([&] { return smx_head_forward(h, w, b, y, R, C, O, nullptr); });
  };
  for (int O : {1, 2}) {
    head_fwd("", H, W, Bv, Y, 37, 96, O);
    head_fwd("b=0", H, W, nullptr, Y, 37, 97, O);
    head_fwd("", H, W, Bv, Y, 100000, 1000, O);
  }
  head_fwd("O=3", H, W, Bv, Y, 37, 96, 3);
  head_fwd("C=1025", H, W, Bv, Y, 37, 1025, 1);
  head_fwd("R=0", H, W, Bv, Y, 0, 96, 1);
  head_fwd("h=0", nullptr, W, Bv, Y, 37, 96, 1);
  head_fwd("y=0", H, W, Bv, nullptr, 37, 96, 1);
  head_fwd("w+8", H, dp("w", 8), Bv, Y, 37, 96, 1);
  head_fwd("y+2", H, W, Bv, dp("y", 2), 37, 96, 1);
  struct HB { const float *g, *h, *w; float *gh, *gw, *gb; };
  const HB all{G, H, W, dp("grad_h"), dp("grad_w"), dp("grad_b")};
  auto head_bwd = [&](const std::string& what, const HB& a, long long R, int C, int O, bool ws_cases = false) {
    const size_t need = sized([&](size_t* n) { return smx_head_workspace_bytes(R, C, O == 3 ? 1 : O, n); });
    const std::string name = fmt("head_backward (%lld,%d) O=%d ", R, C, O) + what;
    auto f = [&](void* ws, size_t n) { return smx_head_backward(a.g, a.h, a.w, a.gh, a.gw, a.gb, ws, n, R, C, O, nullptr); };
    if (ws_cases) return with_ws(name.c_str(), need, f);
    IN("%s", name.c_str());
    call([&] { return f(WS, need); });
  };
  for (int O : {1, 2}) {
    head_bwd("all", all, 37, 96, O, true);
    head_bwd("grad_h only", HB{G, H, W, all.gh, nullptr, nullptr}, 37, 96, O);
    head_bwd("grad_w grad_b only", HB{G, H, W, nullptr, all.gw, all.gb}, 37, 96, O);
    head_bwd("grad_b only, h=0 w=0", HB{G, nullptr, nullptr, nullptr, nullptr, all.gb}, 37, 97, O);
    head_bwd("no gradient", HB{G, H, W, nullptr, nullptr, nullptr}, 37, 96, O);
    head_bwd("all", all, 100000, 1000, O);
  }
  head_bwd("all", all, 37, 96, 3);
  head_bwd("all", all, 37, 1025, 1);
  head_bwd("g=0", HB{nullptr, H, W, all.gh, all.gw, all.gb}, 37, 96, 1);
  head_bwd("h=0 with grad_w", HB{G, nullptr, W, all.gh, all.gw, all.gb}, 37, 96, 1);
  head_bwd("w=0 with grad_h", HB{G, H, nullptr, all.gh, all.gw, all.gb}, 37, 96, 1);
  head_bwd("grad_h+8", HB{G, H, W, dp("grad_h", 8), all.gw, all.gb}, 37, 96, 1);
  head_bwd("grad_w+2", HB{G, H, W, all.gh, dp("grad_w", 2), all.gb}, 37, 96, 1);
  head_bwd("grad_h=h", HB{G, H, W, H, all.gw, all.gb}, 37, 96, 1);
  head_bwd("grad_h=g", HB{G, H, W, G, all.gw, all.gb}, 37, 96, 1);
}

static void xent_and_sampler() {
  float *X = dp("logits"), *G = dp("g"), *LOSS = dp("loss"), *LSE = dp("lse"), *CNT = dp("count"), *GR = dp("grad");
  long long* TG = dp<long long>("targets");
  IN("xent_supported V=-1,0,1,50257");
  answer(fmt("%d%d%d%d", smx_xent_supported(-1), smx_xent_supported(0), smx_xent_supported(1), smx_xent_supported(50257)));
  auto xent_ws = [&](const char* what, long long R, int V, bool out = true) {
    IN("xent_workspace_bytes (%lld,%d) %s", R, V, what);
    query([&](size_t* n) { return smx_xent_workspace_bytes(R, V, out ? n : nullptr); });
  };
  xent_ws("", 37, 256);
  xent_ws("", 5000, 50257);
  xent_ws("out=0", 37, 256, false);
  xent_ws("R=0", 0, 256);
  xent_ws("V=0", 37, 0);
  xent_ws("R=2^31", 1ll << 31, 256);
  struct XF { const float* x; long long stride; const long long* t; int red; float *loss, *lse, *cnt; };
  auto xfwd = [&](const std::string& what, const XF& a, long long R, int V, bool ws_cases = false) {
    const size_t need = sized([&](size_t* n) { return smx_xent_workspace_bytes(R, V, n); });
    const std::string name = fmt("xent_forward (%lld,%d) stride=%lld reduction=%d ", R, V, a.stride, a.red) + what;
    auto f = [&](void* ws, size_t n) {
      return smx_xent_forward(a.x, a.stride, a.t, -100, a.red, a.loss, a.lse, a.cnt, ws, n, R, V, nullptr);
    };
    if (ws_cases) return with_ws(name.c_str(), need, f);
    IN("%s", name.c_str());
    call([&] { return f(WS, need); });
  };
  struct XB { const float *g, *x; long long stride; const long long* t; int red; const float *lse, *cnt; float* grad; };
  auto xbwd = [&](const std::string& what, const XB& a, long long R, int V) {
    IN("xent_backward (%lld,%d) stride=%lld reduction=%d %s", R, V, a.stride, a.red, what.c_str());
    call([&] { return smx_xent_backward(a.g, a.x, a.stride, a.t, -100, a.red, a.lse, a.cnt, a.grad, R, V, nullptr); });
  };
  // the row families: 16-byte register rows; scalar register rows (V % 4, or rows off 16 bytes with V <= 1024); streaming
  // rows (wider than the register rows of their alignment), few and more than the most blocks
  struct Fam { const char* name; long long R; int V; long long stride; int off; };
  const Fam fams[] = {{"vec4 rows", 37, 256, 260, 0},       {"vec4 rows, widest", 37, 4096, 4096, 0},
                      {"scalar rows: V % 4", 37, 255, 300, 0}, {"scalar rows: stride % 4", 37, 256, 257, 0},
                      {"scalar rows: logits+4", 37, 1024, 1024, 4}, {"streaming: V % 4", 37, 50257, 50260, 0},
                      {"streaming: stride % 4", 37, 1028, 1029, 0}, {"streaming: V > 4096", 5000, 4100, 4100, 0}};
  for (const Fam& f : fams)
    for (int red : {0, 1, 2}) {
      if (red && &f != &fams[0] && &f != &fams[5]) continue;
      xfwd(f.name, XF{dp("logits", f.off), f.stride, TG, red, LOSS, LSE, CNT}, f.R, f.V, red == 0 && &f == &fams[0]);
      xbwd(f.name, XB{G, dp("logits", f.off), f.stride, TG, red, LSE, CNT, GR}, f.R, f.V);
    }
  xbwd("grad+4: scalar rows", XB{G, X, 260, TG, 0, LSE, CNT, dp("grad", 4)}, 37, 256);
  const XF xf{X, 260, TG, 0, LOSS, LSE, CNT};
  xfwd("row_stride < V", with<XF>([&](XF& a) { a = xf; a.stride = 255; }), 37, 256);
  xfwd("reduction=3", with<XF>([&](XF& a) { a = xf; a.red = 3; }), 37, 256);
  xfwd("R=0", xf, 0, 256);
  xfwd("R=2^31", xf, 1ll << 31, 256);
  xfwd("logits=0", with<XF>([&](XF& a) { a = xf; a.x = nullptr; }), 37, 256);
  xfwd("lse=0", with<XF>([&](XF& a) { a = xf; a.lse = nullptr; }), 37, 256);
  xfwd("logits+2", with<XF>([&](XF& a) { a = xf; a.x = dp("logits", 2); }), 37, 256);
  xfwd("targets+4", with<XF>([&](XF& a) { a = xf; a.t = dp<long long>("targets", 4); }), 37, 256);
  const XB xb{G, X, 260, TG, 0, LSE, CNT, GR};
  xbwd("row_stride < V", with<XB>([&](XB& a) { a = xb; a.stride = 255; }), 37, 256);
  xbwd("reduction=3", with<XB>([&](XB& a) { a = xb; a.red = 3; }), 37, 256);
  xbwd("V=0", xb, 37, 0);
  xbwd("g=0", with<XB>([&](XB& a) { a = xb; a.g = nullptr; }), 37, 256);
  xbwd("grad=0", with<XB>([&](XB& a) { a = xb; a.grad = nullptr; }), 37, 256);
  xbwd("grad+2", with<XB>([&](XB& a) { a = xb; a.grad = dp("grad", 2); }), 37, 256);
  xbwd("targets+4", with<XB>([&](XB& a) { a = xb; a.t = dp<long long>("targets", 4); }), 37, 256);
  xbwd("grad=logits", with<XB>([&](XB& a) { a = xb; a.grad = X; }), 37, 256);

  IN("sample_supported V=255,256,257");
  answer(fmt("%d%d%d", smx_sample_supported(255), smx_sample_supported(256), smx_sample_supported(257)));
  struct Smp {
    const float* logits = dp("logits"); long long stride = 300; const void* recent = dp<char>("recent"); int tb = 1, n_recent = 8;
    float temp = 0.8f, top_p = 0.9f; int top_k = 40; float rep = 1.1f, pres = 0.1f, freq = 0.2f; int ascii = 1, ban_cr = 1, run = 4;
    const float* u = dp("u"); long long* ids = dp<long long>("ids"); float* probs = dp("probs"); long long R = 5; int V = 256;
  };
  auto smp = [&](const std::string& what, const Smp& a) {
    IN("sample_bytes (%lld,%d) stride=%lld token_bytes=%d n_recent=%d %s", a.R, a.V, a.stride, a.tb, a.n_recent, what.c_str());
    call([&] {
      return smx_sample_bytes(a.logits, a.stride, a.recent, a.tb, a.n_recent, a.temp, a.top_p, a.top_k, a.rep, a.pres, a.freq,
                              a.ascii, a.ban_cr, a.run, a.u, a.ids, a.probs, a.R, a.V, nullptr);
    });
  };
#define SMP(stmt) with<Smp>([&](Smp& a) { stmt; })
  for (int tb : {1, 8})
    for (int nr : {0, 8})
      for (int pr : {0, 1})
        smp(pr ? "probs" : "probs=0", SMP(a.tb = tb; a.n_recent = nr; if (!pr) a.probs = nullptr; if (!nr) a.recent = nullptr));
  smp("plain: top_k=0 top_p=1 no penalties, flags off, n_recent=65536",
      SMP(a.top_k = 0; a.top_p = 1.f; a.rep = 1.f; a.pres = a.freq = 0.f; a.ascii = a.ban_cr = a.run = 0; a.n_recent = 65536));
  smp("R=0", SMP(a.R = 0));
  smp("V=255", SMP(a.V = 255; a.stride = 255));
  smp("R=2^31", SMP(a.R = 1ll << 31));
  smp("logits=0", SMP(a.logits = nullptr));
  smp("u=0", SMP(a.u = nullptr));
  smp("row_stride < V", SMP(a.stride = 255));
  smp("token_bytes=4", SMP(a.tb = 4));
  smp("n_recent=65537", SMP(a.n_recent = 65537));
  smp("n_recent=-1", SMP(a.n_recent = -1));
  smp("recent=0", SMP(a.recent = nullptr));
  smp("recent+4", SMP(a.tb = 8; a.recent = dp<char>("recent", 4)));
  smp("ids+4", SMP(a.ids = dp<long long>("ids", 4)));
  smp("probs+2", SMP(a.probs = dp("probs", 2)));
  smp("temperature=0", SMP(a.temp = 0.f));
  smp("temperature=inf", SMP(a.temp = __builtin_inff()));
  smp("repetition_penalty=0", SMP(a.rep = 0.f));
  smp("top_p=NaN", SMP(a.top_p = __builtin_nanf("")));
  smp("presence_penalty=inf", SMP(a.pres = __builtin_inff()));
  smp("top_k=-1", SMP(a.top_k = -1));
  smp("max_run_length=-1", SMP(a.run = -1));
#undef SMP
}

static void byte_ops() {
  // smx_byte_supported: 1 <= T <= 4096, 0 <= k <= min(T / 2, 2048), 1 <= W <= 4096
  for (int T : {0, 1, 2, 512, 513, 4096, 4097}) {
    IN("byte_supported T=%d: k=-1,0,T/2,T/2+1 x W=0,1,4096,4097", T);
    std::string v;
    for (int k : {-1, 0, T / 2, T / 2 + 1}) {
      for (int W : {0, 1, 4096, 4097}) v += fmt("%d", smx_byte_supported(T, k, W));
      v += " ";
    }
    answer(v);
  }
  struct Feat {
    const void* tokens = dp<char>("tokens"); int tb = 1; long long stride = -1; const float* bands = dp("bands");
    float *out = dp("out"), *mag = dp("mag"); int B = 2, T = 512, k = 32, W = 96, P = -1;
  };
  auto feat = [&](const std::string& what, Feat a) {
    if (a.stride < 0) a.stride = a.T + 8;
    if (a.P < 0) a.P = a.T;
    IN("byte_features (B%d,T%d,k%d,W%d,P%d) token_bytes=%d stride=%lld %s", a.B, a.T, a.k, a.W, a.P, a.tb, a.stride, what.c_str());
    call([&] { return smx_byte_features(a.tokens, a.tb, a.stride, a.bands, a.out, a.mag, a.B, a.T, a.k, a.W, a.P, nullptr); });
  };
#define FEAT(stmt) with<Feat>([&](Feat& a) { stmt; })
  for (int tb : {1, 8})
    for (int W : {96, 97})
      for (int T : {512, 513}) feat("", FEAT(a.tb = tb; a.W = W; a.T = T));
  for (int B : {1, 2, 600, 1024})                           // chunks per row: many ... one
    for (int T : {100, 512, 4096})
      for (int P : {1, T}) feat("", FEAT(a.B = B; a.T = T; a.P = P));
  feat("k=0 bands=0", FEAT(a.k = 0; a.bands = nullptr));
  feat("mag=0", FEAT(a.mag = nullptr));
  for (int k : {1, 3, 4, 5, 64, 128, 255, 256})             // lanes per bin
    feat("", FEAT(a.k = k));
  for (int W : {1, 2, 3, 4, 5, 256, 257, 1024, 1028, 4096}) // threads across a row
    feat("", FEAT(a.W = W));
  feat("widest", FEAT(a.T = 4096; a.k = 2048; a.W = 4096));
  feat("T=1", FEAT(a.T = 1; a.k = 0));
  feat("B=0", FEAT(a.B = 0));
  feat("k=-1", FEAT(a.k = -1));
  feat("token_bytes=4", FEAT(a.tb = 4));
  feat("P=2", FEAT(a.P = 2));
  feat("k > T/2", FEAT(a.k = 257));
  feat("tokens=0", FEAT(a.tokens = nullptr));
  feat("out=0", FEAT(a.out = nullptr));
  feat("bands=0", FEAT(a.bands = nullptr));
  feat("row_stride < T", FEAT(a.stride = 511));
  feat("tokens+4", FEAT(a.tb = 8; a.tokens = dp<char>("tokens", 4)));
  feat("out+8", FEAT(a.out = dp("out", 8)));
  feat("bands+2", FEAT(a.bands = dp("bands", 2)));
  feat("mag+2", FEAT(a.mag = dp("mag", 2)));
  feat("T=4097", FEAT(a.T = 4097));
  feat("W=4097", FEAT(a.W = 4097));
  feat("B*chunks=2^31", FEAT(a.B = 1 << 23; a.T = 4096));
  feat("B*P*W=2^40", FEAT(a.B = 1 << 20; a.T = 4096; a.W = 256));
#undef FEAT

  auto bws = [&](const char* what, int B, int P, int W, int k, bool out = true) {
    IN("byte_workspace_bytes (B%d,P%d,W%d,k%d) %s", B, P, W, k, what);
    query([&](size_t* n) { return smx_byte_workspace_bytes(B, P, W, k, out ? n : nullptr); });
  };
  bws("", 2, 100, 96, 0);
  bws("", 2, 100, 96, 32);
  bws("", 2, 100, 96, 100);
  bws("", 1024, 4096, 4096, 2048);
  bws("", 3, 1, 96, 32);
  bws("out=0", 2, 100, 96, 32, false);
  bws("B=0", 0, 100, 96, 32);
  bws("k=-1", 2, 100, 96, -1);
  struct GB {
    const float *g = dp("g"), *mag = dp("mag"); float* grad = dp("grad_bands"); int n_bands = -1, B = 2, P = 100, W = 96, k = 32;
  };
  auto gb = [&](const std::string& what, GB a, bool ws_cases = false, void* ws = WS) {
    if (a.n_bands < 0) a.n_bands = a.k > 0 ? a.k : 1;
    const size_t need = sized([&](size_t* n) { return smx_byte_workspace_bytes(a.B, a.P, a.W, a.k, n); });
    const std::string name = fmt("byte_grad_bands (B%d,P%d,W%d,k%d) n_bands=%d ", a.B, a.P, a.W, a.k, a.n_bands) + what;
    auto f = [&](void* w, size_t n) {
      return smx_byte_grad_bands(a.g, a.mag, a.grad, a.n_bands, w, n, a.B, a.P, a.W, a.k, nullptr);
    };
    if (ws_cases) return with_ws(name.c_str(), need, f);
    IN("%s", name.c_str());
    call([&] { return f(ws, need); });
  };
#define GBA(stmt) with<GB>([&](GB& a) { stmt; })
  gb("", GB{}, true);
  gb("k=0: ws=0 mag=0", GBA(a.k = 0; a.mag = nullptr), false, nullptr);
  gb("W=1: min(k, W) = 1", GBA(a.W = 1));
  for (int k : {63, 64, 65, 200}) gb("", GBA(a.k = k; a.W = 4096));
  gb("min(k, W) = W", GBA(a.k = 100));
  gb("n_bands > k", GBA(a.n_bands = 300));
  gb("n_bands > k", GBA(a.n_bands = 257));
  gb("P=1", GBA(a.P = 1; a.B = 3));
  gb("P=64", GBA(a.P = 64));
  gb("P=65", GBA(a.P = 65));
  gb("B=0", GBA(a.B = 0));
  gb("k=-1", GBA(a.k = -1; a.n_bands = 1));
  gb("n_bands < min(k, W)", GBA(a.n_bands = 31));
  gb("n_bands=0", GBA(a.k = 0; a.n_bands = 0));
  gb("g=0", GBA(a.g = nullptr));
  gb("grad_bands=0", GBA(a.grad = nullptr));
  gb("mag=0", GBA(a.mag = nullptr));
  gb("g+2", GBA(a.g = dp("g", 2)));
  gb("grad_bands+2", GBA(a.grad = dp("grad_bands", 2)));
  gb("B*P=2^31", GBA(a.B = 1 << 20; a.P = 1 << 17));
#undef GBA
}

static void match_ops() {
  // smx_match_supported: 1 <= S <= 256, 4 <= L <= 256, S L <= 32768 (32769 = 9 * 11 * 331 has no such pair: 99 x 331)
  IN("match_supported S=0,1,128,129,256,257 x L=3,4,128,255,256,257; (99,331)");
  {
    std::string v;
    for (int S : {0, 1, 128, 129, 256, 257}) {
      for (int L : {3, 4, 128, 255, 256, 257}) v += fmt("%d", smx_match_supported(S, L));
      v += " ";
    }
    answer(v + fmt("%d", smx_match_supported(99, 331)));
  }
  auto mws = [&](const char* what, int S, int L, bool out = true) {
    IN("match_workspace_bytes (S%d,L%d) %s", S, L, what);
    query([&](size_t* n) { return smx_match_workspace_bytes(S, L, out ? n : nullptr); });
  };
  mws("", 1, 4);
  mws("", 8, 16);
  mws("", 128, 256);
  mws("", 256, 128);
  mws("out=0", 8, 16, false);
  mws("S*L=33024", 129, 256);
  mws("L=3", 8, 3);
  struct Mt {
    const void* corpus = dp<char>("corpus"); long long n = 1000; const void* snips = dp<char>("snips"); int S = 8, L = 16;
    long long* first = dp<long long>("first"); int max_wg = 0;
  };
  auto mt = [&](const std::string& what, const Mt& a, bool ws_cases = false) {
    const size_t need = sized([&](size_t* n) { return smx_match_workspace_bytes(a.S, a.L, n); });
    const std::string name = fmt("match_first n=%lld (S%d,L%d) max_workgroups=%d ", a.n, a.S, a.L, a.max_wg) + what;
    auto f = [&](void* ws, size_t n) { return smx_match_first(a.corpus, a.n, a.snips, a.S, a.L, a.first, ws, n, a.max_wg, nullptr); };
    if (ws_cases) return with_ws(name.c_str(), need, f);
    IN("%s", name.c_str());
    call([&] { return f(WS, need); });
  };
#define MT(stmt) with<Mt>([&](Mt& a) { stmt; })
  mt("one tile", Mt{}, true);
  mt("corpus=0: the join alone", MT(a.n = 0; a.corpus = nullptr));
  mt("n < L: the join alone", MT(a.n = 15));
  mt("n = L", MT(a.n = 16));
  mt("a full tile", MT(a.n = 16384 + 15));
  mt("one position more", MT(a.n = 16384 + 16));
  mt("off + npos = 16384", MT(a.n = 16394; a.corpus = dp<char>("corpus", 5)));
  mt("off + npos = 16385: a second tile", MT(a.n = 16395; a.corpus = dp<char>("corpus", 5)));
  mt("the same corpus at offset 0: one tile", MT(a.n = 16395));
  mt("corpus+15", MT(a.n = 100; a.corpus = dp<char>("corpus", 15)));
  for (int mw : {0, 1, 2, 2000}) mt("3000 tiles", MT(a.n = 3000ll * 16384; a.max_wg = mw));
  for (long long tiles : {1023, 1024, 1025, 2049})            // around one resident round of four workgroups per CU
    mt(fmt("%lld tiles", tiles), MT(a.n = tiles * 16384));
  // LDS per workgroup: 30976 + S L bytes of 160 KiB: four, three and two workgroups per CU
  const int sls[][2] = {{8, 16}, {128, 160}, {128, 256}, {1, 4}, {256, 128}, {3, 5}};
  for (const auto& sl : sls) mt("3000 tiles: workgroups per CU", MT(a.n = 3000ll * 16384; a.S = sl[0]; a.L = sl[1]));
  mt("L=3", MT(a.L = 3));
  mt("S=257", MT(a.S = 257));
  mt("n=-1", MT(a.n = -1));
  mt("snips=0", MT(a.snips = nullptr));
  mt("first=0", MT(a.first = nullptr));
  mt("corpus=0", MT(a.corpus = nullptr));
  mt("first+4", MT(a.first = dp<long long>("first", 4)));
  mt("max_workgroups=-1", MT(a.max_wg = -1));
#undef MT
}

static void sst_ops() {
  const long long TILE = 4096, NMAX = (1ll << 31) - 1;
  IN("topk_supported n=-1,0,1,2^31-1,2^31");
  answer(fmt("%d%d%d%d%d", smx_topk_supported(-1), smx_topk_supported(0), smx_topk_supported(1), smx_topk_supported(NMAX),
             smx_topk_supported(NMAX + 1)));
  auto tws = [&](const char* what, long long n, bool out = true) {
    IN("topk_workspace_bytes n=%lld %s", n, what);
    query([&](size_t* w) { return smx_topk_workspace_bytes(n, out ? w : nullptr); });
  };
  for (long long n : {1ll, TILE - 2, TILE - 1, TILE, 511 * TILE - 1, 511 * TILE, 512 * TILE, 600 * TILE, NMAX}) tws("", n);
  tws("out=0", 1000, false);
  tws("n=0", 0);
  tws("n=2^31", NMAX + 1);
  struct Tk {
    const void* z = dp<char>("z"); long long n = 10000, k = 100; long long* result = dp<long long>("result");
    void* coeffs = dp<char>("coeffs"); long long* flat_idx = dp<long long>("flat_idx"); long long capacity = 128; int max_wg = 0;
  };
  auto need_of = [&](long long n) { return sized([&](size_t* w) { return smx_topk_workspace_bytes(n, w); }); };
  auto sel = [&](const std::string& what, const Tk& a, bool ws_cases = false) {
    const std::string name = fmt("topk_select n=%lld k=%lld max_workgroups=%d ", a.n, a.k, a.max_wg) + what;
    auto f = [&](void* ws, size_t w) { return smx_topk_select(a.z, a.n, a.k, a.result, ws, w, a.max_wg, nullptr); };
    if (ws_cases) return with_ws(name.c_str(), need_of(a.n), f);
    IN("%s", name.c_str());
    call([&] { return f(WS, need_of(a.n)); });
  };
  auto cmp = [&](const std::string& what, const Tk& a, bool ws_cases = false) {
    const std::string name = fmt("topk_compact n=%lld capacity=%lld max_workgroups=%d ", a.n, a.capacity, a.max_wg) + what;
    auto f = [&](void* ws, size_t w) {
      return smx_topk_compact(a.z, a.n, a.result, a.coeffs, a.flat_idx, a.capacity, ws, w, a.max_wg, nullptr);
    };
    if (ws_cases) return with_ws(name.c_str(), need_of(a.n), f);
    IN("%s", name.c_str());
    call([&] { return f(WS, need_of(a.n)); });
  };
#define TK(stmt) with<Tk>([&](Tk& a) { stmt; })
  sel("", Tk{}, true);
  cmp("", Tk{}, true);
  cmp("capacity=0: nothing launched", TK(a.capacity = 0; a.coeffs = nullptr; a.flat_idx = nullptr), true);
  for (long long n : {1ll, 3 * TILE, 512 * TILE, 513 * TILE, 600 * TILE, 1024 * TILE, 1025 * TILE, 2500 * TILE, NMAX}) {
    sel("", TK(a.n = n; a.k = n == 1 ? 1 : n / 2));
    cmp("", TK(a.n = n));
  }
  // z 8 bytes past a 16-byte boundary: off = 1, one tile more where n fills its tiles
  for (long long n : {1ll, 3 * TILE - 1, 3 * TILE, 512 * TILE}) {
    sel("z+8", TK(a.n = n; a.k = 1; a.z = dp<char>("z", 8)));
    cmp("z+8", TK(a.n = n; a.z = dp<char>("z", 8)));
  }
  for (int mw : {1, 3, 5000}) {
    sel("", TK(a.n = 600 * TILE; a.max_wg = mw));
    cmp("", TK(a.n = 600 * TILE; a.max_wg = mw));
  }
  sel("k=n", TK(a.k = a.n));
  sel("n=0", TK(a.n = 0));
  sel("n=2^31", TK(a.n = NMAX + 1));
  sel("z=0", TK(a.z = nullptr));
  sel("result=0", TK(a.result = nullptr));
  sel("k=0", TK(a.k = 0));
  sel("k=n+1", TK(a.k = a.n + 1));
  sel("z+4", TK(a.z = dp<char>("z", 4)));
  sel("result+4", TK(a.result = dp<long long>("result", 4)));
  sel("max_workgroups=-1", TK(a.max_wg = -1));
  cmp("n=0", TK(a.n = 0));
  cmp("capacity=-1", TK(a.capacity = -1));
  cmp("z=0", TK(a.z = nullptr));
  cmp("result=0", TK(a.result = nullptr));
  cmp("coeffs=0", TK(a.coeffs = nullptr));
  cmp("flat_idx=0", TK(a.flat_idx = nullptr));
  cmp("z+4", TK(a.z = dp<char>("z", 4)));
  cmp("coeffs+4", TK(a.coeffs = dp<char>("coeffs", 4)));
  cmp("flat_idx+4", TK(a.flat_idx = dp<long long>("flat_idx", 4)));
  cmp("max_workgroups=-1", TK(a.max_wg = -1));
#undef TK

  struct Sc {
    const void* coeffs = dp<char>("coeffs"); const long long* flat_idx = dp<long long>("flat_idx"); long long m = 100;
    void* out = dp<char>("out"); long long n = 10 * 4096 + 5; int max_wg = 0;
  };
  auto sc = [&](const std::string& what, const Sc& a) {
    IN("sparse_scatter m=%lld n=%lld max_workgroups=%d %s", a.m, a.n, a.max_wg, what.c_str());
    call([&] { return smx_sparse_scatter(a.coeffs, a.flat_idx, a.m, a.out, a.n, a.max_wg, nullptr); });
  };
#define SC(stmt) with<Sc>([&](Sc& a) { stmt; })
  sc("", Sc{});
  sc("m=0 coeffs=0 flat_idx=0", SC(a.m = 0; a.coeffs = nullptr; a.flat_idx = nullptr));
  sc("m=n", SC(a.m = a.n));
  for (long long n : {1ll, TILE, TILE + 1, 2048 * TILE, 2048 * TILE + 1, 5000 * TILE, NMAX}) sc("", SC(a.n = n; a.m = 1));
  for (int mw : {1, 3, 5000}) sc("", SC(a.n = 5000 * TILE; a.max_wg = mw));
  sc("n=0", SC(a.n = 0; a.m = 0));
  sc("n=2^31", SC(a.n = NMAX + 1));
  sc("m=-1", SC(a.m = -1));
  sc("m=n+1", SC(a.m = a.n + 1));
  sc("out=0", SC(a.out = nullptr));
  sc("coeffs=0", SC(a.coeffs = nullptr));
  sc("flat_idx=0", SC(a.flat_idx = nullptr));
  sc("out+8", SC(a.out = dp<char>("out", 8)));
  sc("coeffs+4", SC(a.coeffs = dp<char>("coeffs", 4)));
  sc("flat_idx+4", SC(a.flat_idx = dp<long long>("flat_idx", 4)));
  sc("max_workgroups=-1", SC(a.max_wg = -1));
#undef SC
}

static void newer_ops() {
  g_last_shape.clear(), puts("## newer ops");
  word_targets_and_head();
  xent_and_sampler();
  byte_ops();
  match_ops();
  sst_ops();
}

// ---- plans ------------------------------------------------------------------------------------------------------------
// plan = path L bands nsplit workgroups groups, the workspace size, sup = row_scale io(bf16) io(f32) block_io(f16)
// block_io(f32); conv (which does not look at F or k) = workspace and save bytes, the cfft workspace, conv conv_io(bf16)
static std::string plan_line(const smx_shape& h, bool conv) {
  std::string s;
  smx_plan p{};
  size_t n = 0, n2 = 0;
  int rc = smx_plan_query_ex(&h, &p);
  s += rc ? fmt("rc=%d", rc) : fmt("%d %d %d %d %d %d", p.path, p.L, p.bands, p.nsplit, p.workgroups, p.groups);
  if (!rc && p.k != h.k) s += fmt(" k=%d", p.k);
  rc = smx_workspace_bytes_ex(&h, &n);
  s += rc ? fmt(" rc=%d", rc) : fmt(" %zu", n);
  if (is_layer(h)) {
    smx_plan q{};
    size_t m = 0;
    const int r1 = smx_plan_query(h.B, h.n_fft, h.D, h.F, &q), r2 = smx_workspace_bytes(h.B, h.n_fft, h.D, h.F, &m);
    if (r1 || r2 || memcmp(&p, &q, sizeof p) || m != n) s += " LAYER-ENTRIES-DIFFER";
  }
  s += fmt(" %d%d%d%d%d", smx_row_scale_supported(&h), smx_io_supported(h.B, h.n_fft, h.D, h.F, 1),
           smx_io_supported(h.B, h.n_fft, h.D, h.F, 0), smx_block_io_supported(h.B, h.n_fft, h.D, h.F, 2),
           smx_block_io_supported(h.B, h.n_fft, h.D, h.F, 0));
  if (!conv) return s;
  rc = smx_conv_workspace_bytes(&h, &n, &n2);
  s += rc ? fmt(" conv rc=%d", rc) : fmt(" conv %zu %zu", n, n2);
  rc = smx_cfft_workspace_bytes(&h, &n);
  s += rc ? fmt(" rc=%d", rc) : fmt(" %zu", n);
  s += fmt(" %d%d", smx_conv_supported(&h), smx_conv_io_supported(&h, 1));
  return s;
}
static void plans() {
  // n_fft: every tile-count class (1, 2, 3, 4: band kernels; 5 ... 32 one-level four-step, 8 also eight bands; 33: band
  // groups; 36 ... two-level; 256 the last; 257 none) and lengths that are no multiple of 256
  const int NS[] = {256, 512, 768, 1024, 1280, 2048, 4096, 8192, 8448, 9216, 16384, 65536, 65792, 100, 400, 1000, 4000, 16000};
  const int BS[] = {1, 2, 8, 64}, DS[] = {2, 34, 64, 256, 257};
  const Opts opts[] = {DEFAULT, FS0, OPT("full8=0", o.full8 = 0), FS0_F80, FORCE_DIRECT, NO_D16, NSPLIT4,
                       OPT("conv1=0", o.conv1 = 0), OPT("conv1=2", o.conv1 = 2), OPT("conv1=3", o.conv1 = 3)};
  std::map<std::string, std::string> base;
  for (const Opts& o : opts) {
    Scope sc(o);
    const bool dflt = &o == &opts[0];
    printf("## plans [%s]: per n_fft, a digest of the lines of the whole grid%s\n", o.name.c_str(),
           g_verbose ? "" : dflt ? "; in full (--verbose: all of them) those of B = 8, D = 64"
                                 : " and how many differ from the default options' (--verbose prints them)");
    for (int N : NS) {
      // F: one, two, four bands, more than 512 bins (every bin: the pair's shape), and rows < n_fft with the Nyquist bin
      const int FS[] = {N / 16, N / 6, N / 3, N};
      unsigned long long hsh = 1469598103934665603ull;
      int differ = 0, count = 0;
      for (int B : BS) for (int D : DS) for (int fi = 0; fi < 5; ++fi) {
        const smx_shape h = fi < 4 ? layer(B, N, D, FS[fi]) : smx_shape{B, N - N / 4, D, N, N, N / 2 + 1};
        const std::string key = shp(h), line = plan_line(h, fi == 0 || fi == 4);
        if (g_verbose || (dflt && B == 8 && D == 64)) printf("%s %s\n", key.c_str(), line.c_str());
        if (dflt) base[key] = line;
        else if (base[key] != line) ++differ;
        for (unsigned char c : key + line) { hsh ^= c; hsh *= 1099511628211ull; }
        ++count;
      }
      if (dflt) printf("n_fft=%d: #%016llx\n", N, hsh);
      else printf("n_fft=%d: #%016llx, %d of %d differ\n", N, hsh, differ, count);
    }
  }
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--verbose")) g_verbose = true;
    else { fprintf(stderr, "usage: api_trace [--verbose]\n"); return 2; }
  }
  plans();
  plan_kinds();
  variants();
  blocks();
  convolution();
  small_ops();
  refusals();
  newer_ops();
  return 0;
}
