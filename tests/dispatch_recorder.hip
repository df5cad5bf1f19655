// Host-only recorder of the kernel selection in csrc/gemm.hip and csrc/attn.hip (tests/test_dispatch_cpu.py).
// hipLaunchKernelGGL is redefined to print the kernel instantiation, the grid, the block and the launch arguments instead of
// launching, then both sources are included as they are: every launch in them goes through that macro.  Built with
// `hipcc --offload-host-only`; needs no GPU.  Reads one call per line from stdin (key=value tokens, see main) and prints what each
// call would have launched and what it returned.
#include <hip/hip_runtime.h>
#include "common.h"
#include <cxxabi.h>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <type_traits>
#include <typeinfo>
#include <vector>

namespace rec {
template <auto K> struct Kern {};   // typeid(Kern<k>) demangles to the kernel's name with its full template arguments

inline std::string kernel_name(const std::type_info& t) {
  int st = 0;
  char* d = abi::__cxa_demangle(t.name(), nullptr, nullptr, &st);
  std::string s = d ? d : t.name();
  free(d);
  const std::string anon = "(anonymous namespace)::";
  size_t p = s.find(anon);
  p = p == std::string::npos ? s.find('&') + 1 : p + anon.size();
  s = s.substr(p);
  // cut the parameter list: the first '(' outside the template argument brackets
  int depth = 0;
  for (size_t i = 0; i < s.size(); ++i) {
    if (s[i] == '<') ++depth;
    else if (s[i] == '>') --depth;
    if ((s[i] == '(' && depth == 0) || depth < 0) { s.resize(i); break; }   // (depth < 0: the '>' that closes Kern<...>)
  }
  return s;
}

template <class T> void log_arg(std::ostream& os, const T& v) {
  char buf[64];
  if constexpr (std::is_floating_point_v<T>) { snprintf(buf, sizeof buf, " %.9g", (double)v); os << buf; }
  else if constexpr (std::is_arithmetic_v<T>) os << ' ' << +v;
  else if constexpr (std::is_pointer_v<T>) { snprintf(buf, sizeof buf, " 0x%llx", (unsigned long long)(uintptr_t)v); os << buf; }
  else log_struct(os, v);            // Epi, GArgs: defined below, after the sources that declare them
}

template <class... A> void launch(const std::type_info& k, dim3 grid, dim3 block, size_t shmem, const A&... a) {
  std::ostringstream os;
  os << kernel_name(k) << " grid=" << grid.x;
  if (grid.y != 1 || grid.z != 1) os << ',' << grid.y << ',' << grid.z;
  os << " block=" << block.x;
  if (block.y != 1 || block.z != 1) os << ',' << block.y << ',' << block.z;
  if (shmem) os << " shmem=" << shmem;
  os << " args:";
  (log_arg(os, a), ...);
  puts(os.str().c_str());
}
}  // namespace rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, shmem, stream, ...) \
  rec::launch(typeid(rec::Kern<kern>), dim3(grid), dim3(block), (size_t)(shmem), __VA_ARGS__)
#undef O2_CHECK_LAUNCH
#define O2_CHECK_LAUNCH() do { } while (0)

namespace rec {
struct Device { int cus, xccs; };
inline const Device& device() {
  static const Device d = [] {
    Device v = {256, 8};
    const char* e = getenv("ORBIT2_RECORDER_DEVICE");
    if (e && sscanf(e, "%dx%d", &v.cus, &v.xccs) != 2) { fprintf(stderr, "ORBIT2_RECORDER_DEVICE: CUSxXCCS\n"); exit(2); }
    return v;
  }();
  return d;
}
inline hipError_t get_device(int* dev) { *dev = 0; return hipSuccess; }
inline hipError_t device_attribute(int* v, hipDeviceAttribute_t attr, int) {
  if (attr == hipDeviceAttributeMultiprocessorCount) { *v = device().cus; return hipSuccess; }
  if (attr == hipDeviceAttributeNumberOfXccs) { *v = device().xccs; return hipSuccess; }
  return hipErrorInvalidValue;
}
}  // namespace rec
#define hipGetDevice rec::get_device
#define hipDeviceGetAttribute rec::device_attribute

#include "gemm.hip"
#include "attn.hip"

namespace {
void log_struct(std::ostream& os, const Epi& e) {
  os << " {";
  rec::log_arg(os, e.bias); rec::log_arg(os, e.save_pre); rec::log_arg(os, e.dgelu_pre); rec::log_arg(os, e.rowscale);
  rec::log_arg(os, e.residual); rec::log_arg(os, e.C); rec::log_arg(os, e.seed);
  for (int v : {e.M, e.N, e.ldc, e.ldr, e.res_mod, e.res_first, e.rows_per_scale, e.act, e.out_fp32}) rec::log_arg(os, v);
  rec::log_arg(os, e.thr); rec::log_arg(os, e.dscale); rec::log_arg(os, e.beta); rec::log_arg(os, e.colscale_n);
  rec::log_arg(os, e.colscale); rec::log_arg(os, e.save_dact); rec::log_arg(os, e.mul); rec::log_arg(os, e.rs_tile);
  rec::log_arg(os, e.colsum_ws); rec::log_arg(os, e.gate); rec::log_arg(os, e.rows_per_gate);
  os << " }";
}
void log_struct(std::ostream& os, const GArgs& g) {
  os << " n=" << g.n << " pace=" << g.pace;
  for (int i = 0; i < g.n; ++i) {
    const GProb& P = g.p[i];
    os << " [";
    rec::log_arg(os, P.A); rec::log_arg(os, P.B);
    for (int v : {P.M, P.N, P.K, P.lda, P.ldb, P.tiles_m, P.tiles_n, P.tile_end}) rec::log_arg(os, v);
    log_struct(os, P.epi);
    rec::log_arg(os, P.kgate); rec::log_arg(os, P.k_per_gate);
    os << " ]";
  }
}

typedef std::map<std::string, std::string> KV;
KV parse(std::istringstream& in) {
  KV kv;
  std::string tok;
  while (in >> tok) {
    const size_t eq = tok.find('=');
    if (eq != std::string::npos) kv[tok.substr(0, eq)] = tok.substr(eq + 1);
  }
  return kv;
}
long long geti(const KV& kv, const char* k, long long dflt) {
  auto it = kv.find(k);
  return it == kv.end() ? dflt : strtoll(it->second.c_str(), nullptr, 0);
}
double getf(const KV& kv, const char* k, double dflt) {
  auto it = kv.find(k);
  return it == kv.end() ? dflt : strtod(it->second.c_str(), nullptr);
}
template <class T = void> T* getp(const KV& kv, const char* k, long long dflt) { return (T*)(uintptr_t)geti(kv, k, dflt); }

orbit2_gemm_args gemm_args(const KV& kv) {          // pointers are fake addresses: nothing on the host dereferences them
  orbit2_gemm_args a = {};
  a.A = getp(kv, "A", 0x10000); a.B = getp(kv, "B", 0x20000); a.C = getp(kv, "C", 0x30000);
  a.M = geti(kv, "M", 0); a.N = geti(kv, "N", 0); a.K = geti(kv, "K", 0);
  a.lda = geti(kv, "lda", 0); a.ldb = geti(kv, "ldb", 0); a.ldc = geti(kv, "ldc", 0);
  a.a_kc = geti(kv, "a_kc", 1); a.b_kc = geti(kv, "b_kc", 1);
  a.bias = getp(kv, "bias", 0); a.act = geti(kv, "act", 0);
  a.save_pre = getp(kv, "save_pre", 0); a.dgelu_pre = getp(kv, "dgelu_pre", 0);
  a.drop_p = (float)getf(kv, "drop_p", 0.0); a.seed = (uint64_t)geti(kv, "seed", 0);
  a.rowscale = getp<const float>(kv, "rowscale", 0); a.rows_per_scale = geti(kv, "rows_per_scale", 0);
  a.residual = getp(kv, "residual", 0);
  a.ldr = geti(kv, "ldr", 0); a.res_mod = geti(kv, "res_mod", 0); a.res_first = geti(kv, "res_first", 0);
  a.out_fp32 = geti(kv, "out_fp32", 0); a.beta = (float)getf(kv, "beta", 0.0); a.tile_hint = geti(kv, "tile_hint", 0);
  a.colscale_n = geti(kv, "colscale_n", 0); a.colscale = (float)getf(kv, "colscale", 1.0);
  a.save_dact = getp(kv, "save_dact", 0); a.mul = getp(kv, "mul", 0);
  a.colsum_ws = getp<float>(kv, "colsum_ws", 0);
  return a;
}
}  // namespace

// gemm K=V...               : orbit2_gemm_bf16_colsum_rows, then orbit2_gemm_bf16 (null=1: a NULL argument block; want_colsum=1:
//                             colsum_ws is set when the first call returned rows)
// group n=N lines=L [null=1]: the next L lines ("g K=V...") are the problems; orbit2_gemm_bf16_grouped(args, N)
// afwd / abwd K=V...        : orbit2_attn_fwd_ld / orbit2_attn_bwd_ld
// Each of them takes the path gate and the tail queue as climate_learn/_hip.py passes them:
//   gate=ADDR rows_per_gate=N : the path gate (attention: gate=ADDR alone); without the key: NULL.  A "g" line: kgate=ADDR
//                               k_per_gate=N, and the group gets the two arrays when any of its lines names one (the others:
//                               NULL, 0); otherwise NULL, NULL
//   sched=ADDR tail=N         : the counter and the tail (0 sized by the library, > 0 that many tiles, < 0 static); without the
//                               sched key: NULL, -1, the plain call
// The sched key decides, whatever its value (sched=0 tail=0: a NULL counter with a tail, which the entries refuse).
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd) || cmd[0] == '#') continue;
    const KV kv = parse(in);
    printf("> %s\n", line.c_str());
    const float* gate = getp<const float>(kv, "gate", 0);
    const int rows_per_gate = (int)geti(kv, "rows_per_gate", 0), tail = kv.count("sched") ? (int)geti(kv, "tail", 0) : -1;
    void* sched = getp(kv, "sched", 0);
    int rc = 0;
    if (cmd == "gemm") {
      orbit2_gemm_args a = gemm_args(kv);
      const orbit2_gemm_args* pa = geti(kv, "null", 0) ? nullptr : &a;
      const int rows = orbit2_gemm_bf16_colsum_rows(pa);
      printf("colsum_rows=%d\n", rows);
      if (geti(kv, "want_colsum", 0) && rows > 0) a.colsum_ws = (float*)0x70000;   // as climate_learn/_hip.py:gemm does
      rc = orbit2_gemm_bf16(pa, gate, rows_per_gate, sched, tail, nullptr);
    } else if (cmd == "group") {
      std::vector<orbit2_gemm_args> v(16);
      const float* kgates[16] = {};
      int kper[16] = {};
      bool kgated = false;
      const int lines = (int)geti(kv, "lines", 0);
      for (int i = 0; i < lines && std::getline(std::cin, line); ++i) {
        std::istringstream gin(line);
        gin >> cmd;
        const KV gkv = parse(gin);
        if (i >= 16) continue;
        v[i] = gemm_args(gkv);
        kgates[i] = getp<const float>(gkv, "kgate", 0);
        kper[i] = (int)geti(gkv, "k_per_gate", 0);
        kgated = kgated || gkv.count("kgate") != 0;
      }
      const orbit2_gemm_args* pv = geti(kv, "null", 0) ? nullptr : v.data();
      const int n = (int)geti(kv, "n", 0);
      rc = orbit2_gemm_bf16_grouped(pv, n, kgated ? kgates : nullptr, kgated ? kper : nullptr, sched, tail, nullptr);
    } else if (cmd == "afwd") {
      void *qkv = getp(kv, "qkv", 0x10000), *out = getp(kv, "out", 0x20000);
      float* lse = getp<float>(kv, "lse", 0x30000);
      const int B = geti(kv, "B", 1), L = geti(kv, "L", 1), H = geti(kv, "H", 1), d = geti(kv, "d", 64), flags = geti(kv, "flags", 0),
                ldq = geti(kv, "ldq", 0), ldo = geti(kv, "ldo", 0);
      const float p = (float)getf(kv, "drop_p", 0.0);
      const uint64_t seed = (uint64_t)geti(kv, "seed", 0);
      rc = orbit2_attn_fwd_ld(qkv, out, lse, B, L, H, d, p, seed, flags, ldq, ldo, gate, sched, tail, nullptr);
    } else if (cmd == "abwd") {
      void *qkv = getp(kv, "qkv", 0x10000), *out = getp(kv, "out", 0x20000), *dout = getp(kv, "dout", 0x40000),
           *dqkv = getp(kv, "dqkv", 0x60000);
      float *lse = getp<float>(kv, "lse", 0x30000), *delta = getp<float>(kv, "delta", 0x50000);
      const int B = geti(kv, "B", 1), L = geti(kv, "L", 1), H = geti(kv, "H", 1), d = geti(kv, "d", 64), flags = geti(kv, "flags", 0),
                ldq = geti(kv, "ldq", 0), ldo = geti(kv, "ldo", 0);
      const float p = (float)getf(kv, "drop_p", 0.0);
      const uint64_t seed = (uint64_t)geti(kv, "seed", 0);
      rc = orbit2_attn_bwd_ld(qkv, out, dout, lse, delta, dqkv, B, L, H, d, p, seed, flags, ldq, ldo, gate, sched, tail, nullptr);
    } else {
      fprintf(stderr, "unknown command: %s\n", cmd.c_str());
      return 2;
    }
    printf("rc=%d\n", rc);
  }
  return 0;
}
