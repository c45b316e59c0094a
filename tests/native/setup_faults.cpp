// setup_faults.cpp -- every failure point of the set-up builders, taken on a CPU.
//
// The builders of appnp_graph.hip, appnp_blocks.hip and appnp_ingest.hip allocate, launch, read a
// count back and allocate again; a mistake on one of their failure paths is a leak, a double free
// or a stale error in the caller's process.  This program links the three units (compiled as
// usual, device code included) against stand-ins for the HIP runtime: allocations are host memory
// and every live one is tracked, memset and memcpy act on it, launches run nothing.  Since no
// kernel runs, the totals the builders read back would all be 0 and their second halves would
// allocate nothing; so the launch stand-in writes a made-up total where the scan's last kernel
// would, and a made-up count where the near-entry kernels would.
//
// Each driver runs once clean, which counts its allocations and synchronisations and checks that
// what is live afterwards is exactly what the graph (or the csr) holds.  Then it runs once per
// allocation with that allocation failing (hipErrorOutOfMemory -> APPNP_ENOMEM) and once per
// synchronisation with that one failing (hipErrorLaunchFailure -> APPNP_EDEVICE), every index in
// turn.  After the clean-up the public entry point performs (graph_free; the csr entry points
// clean up themselves) nothing may be live, and no pointer may have been freed twice or freed
// without having come from the stand-in.  The source-block builder is best-effort: it must also
// leave the last-error slot clear and the graph exactly as it found it.
//
// Prints one line per driver; exits 1 if any check failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "../../ppnp_amd/csrc/appnp_internal.h"

namespace {

std::map<char*, size_t>& live() {  // start -> bytes of every live stand-in allocation
  static std::map<char*, size_t> m;
  return m;
}
std::map<const void*, std::string>& kernels() {  // host stub -> device name
  static std::map<const void*, std::string> m;
  return m;
}

int g_mallocs = 0, g_syncs = 0;          // calls since arm()
int g_fail_malloc = 0, g_fail_sync = 0;  // 1-based index of the call that fails (0: none)
int g_bad = 0;                           // bad frees and out-of-bounds memsets since arm()
hipError_t g_last = hipSuccess;          // the last-error slot
int g_poke_malloc = 0;                   // write g_poke_value into this allocation when made
unsigned g_poke_value = 0;
constexpr int64_t kTotal = 128;          // what every scan "counts"
constexpr unsigned long long kNear = 3;  // what the near-entry kernels "count"

void arm(int fail_malloc, int fail_sync) {
  g_mallocs = g_syncs = g_bad = 0;
  g_fail_malloc = fail_malloc;
  g_fail_sync = fail_sync;
  g_last = hipSuccess;
}

hipError_t fail(hipError_t e) {
  g_last = e;
  return e;
}

bool inside(const void* p, size_t bytes) {
  auto it = live().upper_bound((char*)p);
  if (it == live().begin()) return false;
  --it;
  return (char*)p + bytes <= it->first + it->second;
}

template <class T>
T* arg(void** args, int i) {  // argument i of a launch, a pointer
  return *static_cast<T**>(args[i]);
}

}  // namespace

// ---- the HIP runtime, stood in for -----------------------------------------------------------

hipError_t hipMalloc(void** p, size_t bytes) {
  ++g_mallocs;
  if (g_mallocs == g_fail_malloc || bytes > ((size_t)1 << 28)) return fail(hipErrorOutOfMemory);
  char* m = static_cast<char*>(calloc(bytes ? bytes : 1, 1));
  live()[m] = bytes;
  if (g_mallocs == g_poke_malloc) memcpy(m, &g_poke_value, sizeof(g_poke_value));
  *p = m;
  return hipSuccess;
}

hipError_t hipFree(void* p) {
  if (!p) return hipSuccess;
  auto it = live().find(static_cast<char*>(p));
  if (it == live().end()) {
    ++g_bad;  // freed twice, or never handed out
    return fail(hipErrorInvalidValue);
  }
  live().erase(it);
  free(p);
  return hipSuccess;
}

hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
  if (!inside(dst, bytes)) {
    ++g_bad;
    return fail(hipErrorInvalidValue);
  }
  memset(dst, value, bytes);
  return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  memcpy(dst, src, bytes);
  return hipSuccess;
}

hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  memcpy(dst, src, bytes);
  return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t) {
  return ++g_syncs == g_fail_sync ? fail(hipErrorLaunchFailure) : hipSuccess;
}

hipError_t hipGetLastError() {
  const hipError_t e = g_last;
  g_last = hipSuccess;
  return e;
}

hipError_t hipGetDevice(int* dev) {
  *dev = 0;
  return hipSuccess;
}

int hipGetStreamDeviceId(hipStream_t) { return 0; }

hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t attr, int) {
  *v = attr == hipDeviceAttributeMultiprocessorCount ? 4
       : attr == hipDeviceAttributeWarpSize           ? 64
                                                      : 0;
  return hipSuccess;
}

hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {
  memset(p, 0, sizeof(*p));
  strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
  p->warpSize = 64;
  p->multiProcessorCount = 4;
  p->maxThreadsPerBlock = 1024;
  p->sharedMemPerBlock = 64 * 1024;
  return hipSuccess;
}

hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }

extern "C" void** __hipRegisterFatBinary(const void*) {
  static void* module = nullptr;
  return &module;
}
extern "C" void __hipUnregisterFatBinary(void**) {}
extern "C" void __hipRegisterFunction(void**, const void* host, char*, const char* name, unsigned,
                                      void*, void*, dim3*, dim3*, int*) {
  kernels()[host] = name;
}

namespace {
struct {
  dim3 grid, block;
  size_t lds;
  hipStream_t s;
} g_config;
}  // namespace

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t s) {
  g_config = {grid, block, lds, s};
  return hipSuccess;
}

hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* s) {
  *grid = g_config.grid;
  *block = g_config.block;
  *lds = g_config.lds;
  *s = g_config.s;
  return hipSuccess;
}

hipError_t hipLaunchKernel(const void* host, dim3 grid, dim3, void** args, size_t, hipStream_t) {
  const std::string& name = kernels()[host];
  if (name.empty() || grid.x == 0) {
    ++g_bad;  // an unregistered kernel or an empty grid
    return fail(hipErrorInvalidValue);
  }
  // what the kernels that never run would have counted
  if (name.find("k_scan_spine") != std::string::npos) *arg<int64_t>(args, 2) = kTotal;
  if (name.find("k_near_all") != std::string::npos) *arg<unsigned long long>(args, 3) = kNear;
  if (name.find("k_rb_walkILb0E") != std::string::npos && arg<unsigned long long>(args, 14))
    *arg<unsigned long long>(args, 14) = kNear;
  return hipSuccess;
}

namespace appnp {
int tuning_env(const char*, int dflt) { return dflt; }
}  // namespace appnp

// ---- drivers -----------------------------------------------------------------------------------

namespace {

using appnp::graph_free;

constexpr int64_t kN = 6, kNnz = 10;
const hipStream_t kStream = nullptr;
// inputs the builders only pass on to kernels: never dereferenced on the host
int32_t* const kIndptr = reinterpret_cast<int32_t*>(0x1000);
int32_t* const kIndices = reinterpret_cast<int32_t*>(0x2000);
float* const kVals = reinterpret_cast<float*>(0x3000);

int g_failures = 0;

void check(bool ok, const char* driver, int k_malloc, int k_sync, const char* what) {
  if (ok) return;
  ++g_failures;
  printf("FAIL %s [alloc %d, sync %d]: %s\n", driver, k_malloc, k_sync, what);
}

// A built graph of kN rows as the later builders find it: its arrays come from the stand-in (so
// graph_free may release them), made before the counters are armed.
void make_graph(appnp_graph* g, int mode, int unit, int64_t row_lo, int64_t row_hi) {
  g->n = kN;
  g->row_lo = row_lo;
  g->row_hi = row_hi;
  g->mode = mode;
  g->unit = unit;
  g->nnz_hat = kNnz;
  (void)hipMalloc(&g->dinv, kN * sizeof(double));
  (void)hipMalloc(&g->row_ptr, (row_hi - row_lo + 1) * sizeof(int32_t));
  (void)hipMalloc(&g->col, kNnz * sizeof(int32_t));
  (void)hipMalloc(&g->val, kNnz * sizeof(float));
}

// the pointers a graph holds; after a clean build exactly these are live
size_t held(const appnp_graph& g) {
  const void* ptrs[] = {g.row_ptr, g.col, g.val, g.lrow_ptr, g.lcol, g.lval, g.rrow_ptr, g.rcol,
                        g.rval, g.dinv, g.heavy, g.t_heavy, g.hub, g.t_hub, g.t_row_ptr, g.t_col,
                        g.t_val, g.rb_off, g.rb_ent, g.rb_val, g.rb_dl, g.rb_dr, g.rb_cblk,
                        g.sh_off};
  size_t n = 0;
  for (const void* p : ptrs) n += p && live().count((char*)p) ? 1 : 0;
  return n;
}

struct Run {
  int rc;
  int mallocs, syncs;
};

// One run of a graph driver: set up (unarmed), build (armed), check, release as the caller does.
// best_effort: the source-block builder's contract.
using Build = std::function<int(appnp_graph*)>;
Run run_graph(const char* name, const Build& setup, const Build& build, bool best_effort,
              int k_malloc, int k_sync) {
  appnp_graph g;
  arm(0, 0);
  setup(&g);
  char before[sizeof(appnp_graph)];
  memcpy(before, static_cast<void*>(&g), sizeof(g));
  const size_t live_before = live().size();
  arm(k_malloc, k_sync);
  const int rc = build(&g);
  const Run r{rc, g_mallocs, g_syncs};
  const bool clean = k_malloc == 0 && k_sync == 0;
  if (clean) {
    check(rc == APPNP_OK, name, 0, 0, "clean run failed");
    check(live().size() == held(g), name, 0, 0, "live allocations are not exactly the graph's");
  } else {
    check(k_malloc ? g_mallocs >= k_malloc : g_syncs >= k_sync, name, k_malloc, k_sync,
          "the failing call was never reached");
    check(rc == (k_malloc ? APPNP_ENOMEM : APPNP_EDEVICE), name, k_malloc, k_sync, "return code");
    if (best_effort) {
      check(g_last == hipSuccess, name, k_malloc, k_sync, "a stale error in the last-error slot");
      check(memcmp(before, static_cast<void*>(&g), sizeof(g)) == 0, name, k_malloc, k_sync,
            "the graph was not left as found");
      check(live().size() == live_before, name, k_malloc, k_sync, "the failed copy leaked");
    }
  }
  graph_free(&g);
  check(live().empty(), name, k_malloc, k_sync, "allocations live after graph_free");
  check(g_bad == 0, name, k_malloc, k_sync, "a bad free or an out-of-bounds memset");
  for (auto& kv : live()) free(kv.first);  // a leak is reported once, not at every later index
  live().clear();
  return r;
}

// One run of a csr driver (the public entry points, which release the csr on failure themselves).
using BuildCsr = std::function<int(appnp_csr**)>;
Run run_csr(const char* name, const BuildCsr& build, size_t held_clean, int k_malloc, int k_sync) {
  appnp_csr* c = nullptr;
  arm(k_malloc, k_sync);
  const int rc = build(&c);
  const Run r{rc, g_mallocs, g_syncs};
  if (k_malloc == 0 && k_sync == 0) {
    check(rc == APPNP_OK && c, name, 0, 0, "clean run failed");
    check(live().size() == held_clean, name, 0, 0, "live allocations are not exactly the csr's");
  } else {
    check(k_malloc ? g_mallocs >= k_malloc : g_syncs >= k_sync, name, k_malloc, k_sync,
          "the failing call was never reached");
    check(rc == (k_malloc ? APPNP_ENOMEM : APPNP_EDEVICE) && !c, name, k_malloc, k_sync,
          "return code");
  }
  appnp_csr_destroy(c);
  check(live().empty(), name, k_malloc, k_sync, "allocations live after the clean-up");
  check(g_bad == 0, name, k_malloc, k_sync, "a bad free or an out-of-bounds memset");
  for (auto& kv : live()) free(kv.first);
  live().clear();
  return r;
}

// The clean run, then every allocation and every synchronisation failing in turn.
template <class RunAt>
void sweep(const char* name, const RunAt& run_at) {
  const int before = g_failures;
  const Run clean = run_at(0, 0);
  for (int k = 1; k <= clean.mallocs; ++k) run_at(k, 0);
  for (int j = 1; j <= clean.syncs; ++j) run_at(0, j);
  printf("%-34s allocs %2d syncs %2d  %s\n", name, clean.mallocs, clean.syncs,
         g_failures == before ? "ok" : "FAILED");
}

void sweep_graph(const char* name, const Build& setup, const Build& build,
                 bool best_effort = false) {
  sweep(name, [&](int k, int j) { return run_graph(name, setup, build, best_effort, k, j); });
}

void sweep_csr(const char* name, const BuildCsr& build, size_t held_clean) {
  sweep(name, [&](int k, int j) { return run_csr(name, build, held_clean, k, j); });
}

}  // namespace

int main() {
  const Build nothing = [](appnp_graph*) { return 0; };
  const Build full_graph = [](appnp_graph* g) {
    make_graph(g, APPNP_NORM_SYM, 1, 0, kN);
    return 0;
  };

  sweep_graph("build_heavy", full_graph, [](appnp_graph* g) {
    return appnp::build_heavy(g->row_ptr, kN, 2, kStream, &g->heavy, &g->n_heavy);
  });
  sweep_graph("graph_build", nothing, [](appnp_graph* g) {
    return appnp::graph_build(kIndptr, kIndices, kVals, kN, kNnz, APPNP_NORM_SYM, 0, kN, 0,
                              kStream, g);
  });
  sweep_graph("graph_build split", nothing, [](appnp_graph* g) {
    return appnp::graph_build(kIndptr, kIndices, nullptr, kN, kNnz, APPNP_NORM_RW, 2, 5, 1,
                              kStream, g);
  });
  sweep_graph("shard_offsets first", full_graph, [](appnp_graph* g) {
    return appnp::graph_build_shard_offsets(g, 2, 3, kStream);
  });
  sweep_graph("shard_offsets replacing",
              [](appnp_graph* g) {
                make_graph(g, APPNP_NORM_SYM, 1, 0, kN);
                return appnp::graph_build_shard_offsets(g, 2, 3, kStream);
              },
              [](appnp_graph* g) { return appnp::graph_build_shard_offsets(g, 3, 2, kStream); });
  for (int mode : {APPNP_NORM_SYM, APPNP_NORM_RW})
    for (int unit : {1, 0})
      for (int lpe : {1, 4}) {
        char name[64];
        snprintf(name, sizeof(name), "source_blocks %s %s w%d", unit ? "unit" : "weighted",
                 mode == APPNP_NORM_SYM ? "sym" : "rw", 4 * lpe);
        sweep_graph(name, [=](appnp_graph* g) { make_graph(g, mode, unit, 0, kN); return 0; },
                    [=](appnp_graph* g) {
                      return appnp::graph_build_source_blocks(g, lpe, kIndptr, kIndices, kNnz,
                                                              kStream);
                    },
                    true);
      }
  sweep_graph("source_blocks unit sym held rows",
              [](appnp_graph* g) { make_graph(g, APPNP_NORM_SYM, 1, 2, 5); return 0; },
              [](appnp_graph* g) {
                return appnp::graph_build_source_blocks(g, 1, kIndptr, kIndices, kNnz, kStream);
              },
              true);
  sweep_graph("graph_build_transpose", full_graph, [](appnp_graph* g) {
    return appnp::graph_build_transpose(g, kStream);
  });

  // standardize: the 4th allocation is the unique-key count, which no kernel writes here; with LCC
  // selection it is made to read 5, so the hooking sweep and its read-back are reached
  sweep_csr("standardize", [](appnp_csr** c) {
    return appnp_standardize(kIndptr, kIndices, nullptr, kN, kNnz, 0, nullptr, c);
  }, 3);
  g_poke_malloc = 4;
  g_poke_value = 5;
  sweep_csr("standardize lcc", [](appnp_csr** c) {
    return appnp_standardize(kIndptr, kIndices, nullptr, kN, kNnz, 1, nullptr, c);
  }, 3);
  g_poke_malloc = 0;
  sweep_csr("csr_transpose", [](appnp_csr** c) {
    return appnp_csr_transpose(kIndptr, kIndices, nullptr, kN, kN, kNnz, nullptr, c);
  }, 2);
  sweep_csr("csr_transpose values", [](appnp_csr** c) {
    return appnp_csr_transpose(kIndptr, kIndices, kVals, kN, kN, kNnz, nullptr, c);
  }, 3);

  printf("%s\n", g_failures ? "FAILED" : "all clean");
  return g_failures ? 1 : 0;
}
