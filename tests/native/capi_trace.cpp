// capi_trace.cpp -- the launch trace of ppnp_amd/csrc/appnp_capi.hip and appnp_propagate.hip,
// recorded on a CPU.
//
// Neither unit holds a kernel: all they do is validate arguments, carve the workspace and
// request launches from the other units.  This program links their host-only objects against
// recording stand-ins for the internal functions they import and for the few HIP runtime calls
// they make, calls the public entry points on fabricated graphs (every pointer a fixed integer,
// nothing is dereferenced, no device is touched) and prints each requested launch with every
// argument, plus each return code.  tests/test_capi_trace.py compares the output with
// tests/golden/capi_trace.txt byte for byte.
//
// Run it with every APPNP_* variable removed from the environment (the units cache overrides).
//
// dist_trace.cpp, the same for appnp_dist.hip, includes this file with TRACE_STANDINS_ONLY set and
// so shares the stand-ins and operands, up to the marked line, without this program's cases.
#include <cinttypes>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "../../ppnp_amd/csrc/appnp_internal.h"

namespace {

unsigned long long X(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

template <typename T>
T* at(uintptr_t v) {
  return reinterpret_cast<T*>(v);
}

uintptr_t g_next_handle = 0xe0000000u;
void* new_handle() {
  g_next_handle += 0x10;
  return at<void>(g_next_handle);
}

// What dist_trace.cpp turns: by default every stand-in prints its call with every argument and
// succeeds, and device-to-host copies write nothing.
bool g_brief = false;   // one short line per call instead of every argument
int g_launches = 0;     // launches (and 2-D copies) requested so far
int g_fail_launch = 0;  // the launch (1-based count) that fails; 0: none
// the byte the device-to-host copy of rank p's agreement flag delivers ("what the peers said")
const unsigned char* g_peer_flags = nullptr;
int g_peer_next = 0;

// the end of a launch's line, and what the launch returns
hipError_t launched() {
  const bool fails = ++g_launches == g_fail_launch;
  printf(fails ? " -> fails\n" : "\n");
  return fails ? hipErrorLaunchFailure : hipSuccess;
}

// what G(flags) fills, for the builders' stand-ins: the held rows, the local / remote halves when
// `split` is set, the source-blocked copy for lpe = 1, 2, 4 (0: none)
void fabricate(appnp_graph* g, int mode, bool split, int lpe, int64_t n, int64_t row_lo,
               int64_t row_hi);

}  // namespace

// ---- recording stand-ins: the units' imports ----------------------------------------------

namespace appnp {

int pick_vec(int dtype, int64_t f, const int64_t* lds, int n_ld, const void* const* ptrs,
             int n_ptr) {
  const int es = dtype == 0 ? 4 : 2;
  int v = dtype == 0 ? 4 : 8;
  for (; v > 1; v >>= 1) {
    bool ok = v <= f || (f % v) == 0;
    for (int i = 0; i < n_ld && ok; ++i) ok = (lds[i] % v) == 0;
    for (int i = 0; i < n_ptr && ok; ++i)
      ok = ptrs[i] == nullptr || (reinterpret_cast<uintptr_t>(ptrs[i]) % (uintptr_t)(v * es)) == 0;
    if (ok) break;
  }
  if (g_brief) return v;
  printf("pick_vec dtype=%d f=%" PRId64 " lds=[", dtype, f);
  for (int i = 0; i < n_ld; ++i) printf("%s%" PRId64, i ? "," : "", lds[i]);
  printf("] ptrs=[");
  for (int i = 0; i < n_ptr; ++i) printf("%s%#llx", i ? "," : "", X(ptrs[i]));
  printf("] -> %d\n", v);
  return v;
}

static void print_args(const StepArgs& a) {
  printf(" row_ptr=%#llx row_end=%#llx col=%#llx val=%#llx zin=%#llx h=%#llx out=%#llx aux=%#llx"
         " ld_in=%" PRId64 " ld_h=%" PRId64 " ld_out=%" PRId64 " ld_aux=%" PRId64
         " n_rows=%" PRId64 " nnz=%" PRId64 " nnz_rows=%" PRId64 " zin_rows=%" PRId64
         " row_lo=%" PRId64 " mkey=%#" PRIx64 " f=%d drop_thr=%u drop_on=%d scale=%a alpha=%a"
         " drop_scale=%a tkey=%d heavy=%#llx n_heavy=%" PRId64 " heavy_thr=%d hub=%#llx"
         " n_hub=%" PRId64 " rem_dh=%#llx ld_rem_dh=%" PRId64 " omega=%a",
         X(a.row_ptr), X(a.row_end), X(a.col), X(a.val), X(a.zin), X(a.h), X(a.out), X(a.aux),
         a.ld_in, a.ld_h, a.ld_out, a.ld_aux, a.n_rows, a.nnz, a.nnz_rows, a.zin_rows, a.row_lo,
         a.mkey, a.f, a.drop_thr, a.drop_on, (double)a.scale, (double)a.alpha,
         (double)a.drop_scale, a.tkey, X(a.heavy), a.n_heavy, a.heavy_thr, X(a.hub), a.n_hub,
         X(a.rem_dh), a.ld_rem_dh, (double)a.omega);
}

hipError_t launch_step(int dtype, int epi, int V, const StepArgs& a, hipStream_t s) {
  if (g_brief) {
    printf("step s=%#llx epi=%d rows=%#llx:%#llx zin=%#llx out=%#llx aux=%#llx", X(s), epi,
           X(a.row_ptr), X(a.row_end), X(a.zin), X(a.out), X(a.aux));
    return launched();
  }
  printf("launch_step dtype=%d epi=%d V=%d s=%#llx", dtype, epi, V, X(s));
  print_args(a);
  return launched();
}

hipError_t launch_remainder(const appnp_graph* g, const StepArgs& a, int epi, const float* z_rem,
                            const float* h_rem, int64_t ld_h, float* out, int64_t ld_out, int nv,
                            bool to_rem, hipStream_t s) {
  if (g_brief) {
    printf("remainder s=%#llx z_rem=%#llx out=%#llx to_rem=%d", X(s), X(z_rem), X(out),
           (int)to_rem);
    return launched();
  }
  printf("launch_remainder lpe=%d epi=%d z_rem=%#llx h_rem=%#llx ld_h=%" PRId64
         " out=%#llx ld_out=%" PRId64 " nv=%d to_rem=%d s=%#llx",
         g->rb_lpe, epi, X(z_rem), X(h_rem), ld_h, X(out), ld_out, nv, (int)to_rem, X(s));
  print_args(a);
  return launched();
}

hipError_t launch_split_copy(const float* h, int64_t ld_h, int64_t n, int64_t f, int64_t fs,
                             int64_t rw, float* main, float* rem, const float* rem_scale,
                             hipStream_t s) {
  if (g_brief) {
    printf("split_copy s=%#llx main=%#llx rem=%#llx", X(s), X(main), X(rem));
    return launched();
  }
  printf("launch_split_copy h=%#llx ld_h=%" PRId64 " n=%" PRId64 " f=%" PRId64 " fs=%" PRId64
         " rw=%" PRId64 " main=%#llx rem=%#llx rem_scale=%#llx s=%#llx",
         X(h), ld_h, n, f, fs, rw, X(main), X(rem), X(rem_scale), X(s));
  return launched();
}

hipError_t launch_scale_rows(int dtype, const void* src, int64_t ld_src, void* dst,
                             int64_t ld_dst, int64_t n, int64_t f, float alpha, hipStream_t s) {
  printf("launch_scale_rows dtype=%d src=%#llx ld_src=%" PRId64 " dst=%#llx ld_dst=%" PRId64
         " n=%" PRId64 " f=%" PRId64 " alpha=%a s=%#llx\n",
         dtype, X(src), ld_src, X(dst), ld_dst, n, f, (double)alpha, X(s));
  return hipSuccess;
}

// the polynomial calls' launches: the step that also reports its column slabs (64 columns each
// here), the row pass of coef[0] and the reduce of the partial dots
int64_t poly_max_slabs(int64_t f) { return (f + 63) / 64; }

hipError_t launch_step_slabs(int dtype, int epi, int V, const StepArgs& a, hipStream_t s,
                             int64_t* slabs_out) {
  printf("launch_step_slabs dtype=%d epi=%d V=%d s=%#llx coef=%#llx coef0=%#llx dots=%#llx", dtype,
         epi, V, X(s), X(a.coef), X(a.coef0), X(a.dots));
  print_args(a);
  printf("\n");
  if (slabs_out) *slabs_out = poly_max_slabs(a.f);
  return hipSuccess;
}

hipError_t launch_poly_rows(const float* src, int64_t ld_src, float* dst, int64_t ld_dst,
                            const float* h, int64_t ld_h, float* dots, int64_t n, int64_t f,
                            const float* coef, hipStream_t s) {
  printf("launch_poly_rows src=%#llx ld_src=%" PRId64 " dst=%#llx ld_dst=%" PRId64
         " h=%#llx ld_h=%" PRId64 " dots=%#llx n=%" PRId64 " f=%" PRId64 " coef=%#llx s=%#llx\n",
         X(src), ld_src, X(dst), ld_dst, X(h), ld_h, X(dots), n, f, X(coef), X(s));
  return hipSuccess;
}

hipError_t launch_poly_reduce(const float* part, int64_t count, float* out, hipStream_t s) {
  printf("launch_poly_reduce part=%#llx count=%" PRId64 " out=%#llx s=%#llx\n", X(part), count,
         X(out), X(s));
  return hipSuccess;
}

int g_build_rc = APPNP_OK;  // what the graph_build_source_blocks stand-in returns

// The builders fabricate what they are asked for, as G(flags) does.

int graph_build(const int32_t* indptr, const int32_t* indices, const float* vals, int64_t n,
                int64_t nnz, int mode, int64_t row_lo, int64_t row_hi, int split, hipStream_t s,
                appnp_graph* g) {
  printf("graph_build indptr=%#llx indices=%#llx vals=%#llx n=%" PRId64 " nnz=%" PRId64
         " mode=%d row_lo=%" PRId64 " row_hi=%" PRId64 " split=%d s=%#llx\n",
         X(indptr), X(indices), X(vals), n, nnz, mode, row_lo, row_hi, split, X(s));
  fabricate(g, mode, split != 0, 0, n, row_lo, row_hi);
  return APPNP_OK;
}

int graph_build_transpose(appnp_graph*, hipStream_t s) {
  printf("graph_build_transpose s=%#llx\n", X(s));
  return APPNP_OK;
}

int graph_build_source_blocks(appnp_graph* g, int lpe, const int32_t* a_indptr,
                              const int32_t* a_indices, int64_t a_nnz, hipStream_t s) {
  printf("graph_build_source_blocks lpe=%d a_indptr=%#llx a_indices=%#llx a_nnz=%" PRId64
         " s=%#llx -> %d\n",
         lpe, X(a_indptr), X(a_indices), a_nnz, X(s), g_build_rc);
  if (g_build_rc == APPNP_OK)
    fabricate(g, g->mode, g->split != 0, lpe, g->n, g->row_lo, g->row_hi);
  return g_build_rc;
}

int graph_build_shard_offsets(appnp_graph* g, int nshards, int64_t shard_rows, hipStream_t s) {
  printf("graph_build_shard_offsets nshards=%d shard_rows=%" PRId64 " s=%#llx\n", nshards,
         shard_rows, X(s));
  g->sh_off = at<int32_t>(0x19000000);
  g->sh_n = nshards;
  g->sh_rows = shard_rows;
  return APPNP_OK;
}

void graph_free(appnp_graph*) { printf("graph_free\n"); }

}  // namespace appnp

// ---- recording stand-ins: the HIP runtime calls of the units -------------------------------

hipError_t hipEventCreate(hipEvent_t* e) {
  *e = static_cast<hipEvent_t>(new_handle());
  printf("hipEventCreate -> %#llx\n", X(*e));
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int flags) {
  *e = static_cast<hipEvent_t>(new_handle());
  printf("hipEventCreateWithFlags flags=%u -> %#llx\n", flags, X(*e));
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  printf("hipEventDestroy %#llx\n", X(e));
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  printf(g_brief ? "record %#llx s=%#llx\n" : "hipEventRecord %#llx s=%#llx\n", X(e), X(s));
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
  printf("hipEventSynchronize %#llx\n", X(e));
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  printf("hipEventElapsedTime %#llx %#llx\n", X(a), X(b));
  *ms = 1.0f;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind,
                          hipStream_t s) {
  if (g_peer_flags && kind == hipMemcpyDeviceToHost && bytes == 1) {
    // the agreement reads rank p's flag into host memory: the address is the run's, not printed
    const unsigned char v = g_peer_flags[g_peer_next++];
    *static_cast<unsigned char*>(dst) = v;
    printf("hipMemcpyAsync dst=host src=%#llx bytes=1 kind=%d s=%#llx -> %d\n", X(src), (int)kind,
           X(s), (int)v);
    return hipSuccess;
  }
  printf("hipMemcpyAsync dst=%#llx src=%#llx bytes=%zu kind=%d s=%#llx\n", X(dst), X(src), bytes,
         (int)kind, X(s));
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch,
                            size_t width, size_t height, hipMemcpyKind kind, hipStream_t s) {
  if (g_brief) {
    printf("copy2d s=%#llx dst=%#llx src=%#llx", X(s), X(dst), X(src));
    return launched();
  }
  printf("hipMemcpy2DAsync dst=%#llx dpitch=%zu src=%#llx spitch=%zu width=%zu height=%zu kind=%d"
         " s=%#llx",
         X(dst), dpitch, X(src), spitch, width, height, (int)kind, X(s));
  return launched();
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) {
  printf("hipMemsetAsync dst=%#llx value=%d bytes=%zu s=%#llx\n", X(dst), value, bytes, X(s));
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int flags) {
  *s = static_cast<hipStream_t>(new_handle());
  printf("hipStreamCreateWithFlags flags=%u -> %#llx\n", flags, X(*s));
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  printf("hipStreamDestroy %#llx\n", X(s));
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  printf("hipStreamSynchronize %#llx\n", X(s));
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int flags) {
  if (g_brief)
    printf("wait s=%#llx %#llx\n", X(s), X(e));
  else
    printf("hipStreamWaitEvent s=%#llx %#llx flags=%u\n", X(s), X(e), flags);
  return hipSuccess;
}
hipError_t hipStreamBeginCapture(hipStream_t s, hipStreamCaptureMode mode) {
  printf("hipStreamBeginCapture %#llx mode=%d\n", X(s), (int)mode);
  return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t s, hipGraph_t* graph) {
  *graph = static_cast<hipGraph_t>(new_handle());
  printf("hipStreamEndCapture %#llx -> %#llx\n", X(s), X(*graph));
  return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t* exec, hipGraph_t graph, hipGraphNode_t*, char*,
                               size_t) {
  *exec = static_cast<hipGraphExec_t>(new_handle());
  printf("hipGraphInstantiate %#llx -> %#llx\n", X(graph), X(*exec));
  return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t exec, hipStream_t s) {
  printf("hipGraphLaunch %#llx s=%#llx\n", X(exec), X(s));
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t exec) {
  printf("hipGraphExecDestroy %#llx\n", X(exec));
  return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t graph) {
  printf("hipGraphDestroy %#llx\n", X(graph));
  return hipSuccess;
}

// ---- fabricated graphs and operands --------------------------------------------------------

namespace {

enum : unsigned {
  G_SMALL = 0x1,     // n = 1000 (latency regime) instead of 200000
  G_RW = 0x2,        // APPNP_NORM_RW
  G_ASYM = 0x4,      // A is not symmetric
  G_TR = 0x8,        // A_hat^T held (distinct t_* arrays)
  G_SB4 = 0x10,      // source-blocked copy, remainder rows of 4 columns
  G_SB8 = 0x20,      // ... of 8
  G_SB16 = 0x40,     // ... of 16
  G_UNIT = 0x80,     // the copy is value-free (rb_val null, rb_dl / rb_dr set)
  G_NEAR = 0x100,    // gather locality: near_frac = 0.9
  G_ROWS = 0x200,    // holds rows [n / 4, 3 n / 4) only
  G_SPLIT = 0x400,   // local / remote half CSRs
  G_SHARDS = 0x800,  // shard offsets, sh_n = 3
  G_EMPTY = 0x1000,  // holds no row
};

// rows [row_lo, row_hi) of an n-node graph with the parts `fl` names
void fill(appnp_graph* g, unsigned fl, int64_t n, int64_t row_lo, int64_t row_hi) {
  g->n = n;
  g->row_lo = row_lo;
  g->row_hi = row_hi;
  g->nnz_hat = 25 * (g->row_hi - g->row_lo) + 3;
  g->mode = (fl & G_RW) ? APPNP_NORM_RW : APPNP_NORM_SYM;
  g->symmetric = (fl & G_ASYM) ? 0 : 1;
  g->unit = (fl & G_UNIT) ? 1 : 0;
  g->row_ptr = at<int32_t>(0x10000000);
  g->col = at<int32_t>(0x11000000);
  g->val = at<float>(0x12000000);
  g->dinv = at<double>(0x13000000);
  g->heavy = at<int32_t>(0x14000000);
  g->n_heavy = 77;
  g->hub = at<int32_t>(0x14100000);
  g->n_hub = 5;
  if (fl & G_SPLIT) {
    g->split = 1;
    g->nnz_local = 15 * (g->row_hi - g->row_lo) + 1;
    g->nnz_remote = g->nnz_hat - g->nnz_local;
    g->lrow_ptr = at<int32_t>(0x15000000);
    g->lcol = at<int32_t>(0x15100000);
    g->lval = at<float>(0x15200000);
    g->rrow_ptr = at<int32_t>(0x16000000);
    g->rcol = at<int32_t>(0x16100000);
    g->rval = at<float>(0x16200000);
  }
  if (fl & G_TR) {
    g->t_row_ptr = at<int32_t>(0x17000000);
    g->t_col = at<int32_t>(0x17100000);
    g->t_val = at<float>(0x17200000);
    g->t_heavy = at<int32_t>(0x17300000);
    g->t_n_heavy = 66;
    g->t_hub = at<int32_t>(0x17400000);
    g->t_n_hub = 4;
  }
  if (fl & (G_SB4 | G_SB8 | G_SB16)) {
    g->rb_lpe = (fl & G_SB16) ? 4 : (fl & G_SB8) ? 2 : 1;
    g->rb_off = at<int32_t>(0x18000000);
    g->rb_ent = at<uint32_t>(0x18100000);
    g->rb_cblk = at<int32_t>(0x18200000);
    if (fl & G_UNIT) {
      g->rb_dl = at<float>(0x18300000);
      if (!(fl & G_RW)) g->rb_dr = at<float>(0x18400000);
    } else {
      g->rb_val = at<float>(0x18500000);
    }
    g->rb_total = 6400000;
    g->rb_nb = 7;
    g->rb_br_log2 = 15;
    g->rb_grid = 256;
    g->rb_slots = 1024;
    g->rb_rg = 16;
    g->rb_passes = 13;
  }
  if (fl & G_SHARDS) {
    g->sh_off = at<int32_t>(0x19000000);
    g->sh_n = 3;
    g->sh_rows = (g->n + 2) / 3;
  }
  g->near_frac = (fl & G_NEAR) ? 0.9 : 0.013;
}

void fabricate(appnp_graph* g, int mode, bool split, int lpe, int64_t n, int64_t row_lo,
               int64_t row_hi) {
  fill(g, (mode == APPNP_NORM_RW ? G_RW : 0u) | (split ? G_SPLIT : 0u) |
              (lpe == 4 ? G_SB16 : lpe == 2 ? G_SB8 : lpe == 1 ? G_SB4 : 0u),
       n, row_lo, row_hi);
}

void* const kH = at<void>(0x20000000);
void* const kZ = at<void>(0x30000000);
void* const kWs = at<void>(0x40000000);
void* const kStream = at<void>(0x5ee0);

template <typename T>
T* off(T* p, intptr_t bytes) {
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + bytes);
}

}  // namespace

#ifndef TRACE_STANDINS_ONLY  // dist_trace.cpp includes what is above; the rest is this program's

namespace {

std::vector<std::unique_ptr<appnp_graph>> g_graphs;  // of the running case

appnp_graph* G(unsigned fl) {
  g_graphs.emplace_back(new appnp_graph());
  appnp_graph* g = g_graphs.back().get();
  const int64_t n = (fl & G_SMALL) ? 1000 : 200000;
  const int64_t lo = (fl & (G_ROWS | G_EMPTY)) ? n / 4 : 0;
  fill(g, fl, n, lo, (fl & G_EMPTY) ? lo : (fl & G_ROWS) ? 3 * n / 4 : n);
  return g;
}

float* const kPartial = at<float>(0x50000000);
float* const kZinMain = at<float>(0x60000000);
float* const kZinRem = at<float>(0x61000000);
float* const kZoutMain = at<float>(0x62000000);
float* const kZoutRem = at<float>(0x63000000);

// appnp_propagate / _bwd / appnp_solve / _bwd / appnp_plan_create(_solve): H, Z are dZ, dH in
// the adjoints; K is `iters` in the solver
struct Prop {
  const appnp_graph* g;
  const void* H = kH;
  int64_t ld_h;
  void* Z = kZ;
  int64_t ld_z;
  int64_t f;
  int dtype = APPNP_F32;
  int K = 3;
  float alpha = 0.1f, p_drop = 0.0f;
  uint64_t seed = 42;
  void* ws = kWs;
  size_t ws_bytes;
  void* stream = kStream;

  Prop(const appnp_graph* g_, int64_t f_, int dtype_ = APPNP_F32)
      : g(g_), ld_h(f_), ld_z(f_), f(f_), dtype(dtype_),
        ws_bytes(appnp_workspace_bytes(g_, f_, f_, dtype_)) {}
  int fwd() const {
    return appnp_propagate(g, H, ld_h, Z, ld_z, f, dtype, K, alpha, p_drop, seed, ws, ws_bytes,
                           stream);
  }
  int bwd() const {
    return appnp_propagate_bwd(g, H, ld_h, Z, ld_z, f, dtype, K, alpha, p_drop, seed, ws,
                               ws_bytes, stream);
  }
  int solve() const {
    return appnp_solve(g, H, ld_h, Z, ld_z, f, dtype, K, alpha, ws, ws_bytes, stream);
  }
  int solve_bwd() const {
    return appnp_solve_bwd(g, H, ld_h, Z, ld_z, f, dtype, K, alpha, ws, ws_bytes, stream);
  }
  // create, launch and destroy the plan
  int plan(bool solver) const {
    appnp_plan* p = at<appnp_plan>(0xbad0);
    const int rc = solver ? appnp_plan_create_solve(g, H, ld_h, Z, ld_z, f, dtype, K, alpha, ws,
                                                    ws_bytes, &p)
                          : appnp_plan_create(g, H, ld_h, Z, ld_z, f, dtype, K, alpha, p_drop,
                                              seed, ws, ws_bytes, &p);
    printf("plan=%s\n", p ? (p == at<appnp_plan>(0xbad0) ? "untouched" : "set") : "null");
    if (rc == APPNP_OK) {
      printf("appnp_plan_launch -> %d\n", appnp_plan_launch(p, kStream));
      appnp_plan_destroy(p);
    }
    return rc;
  }
};

// appnp_poly / appnp_poly_bwd: X, Y are H, Z in the forward and dZ, dH in the adjoint, which
// reads H (kPartial's address stands in) and writes dcoef where it is not null
struct Poly {
  const appnp_graph* g;
  const void* X = kH;
  int64_t ld_x;
  void* Y = kZ;
  int64_t ld_y;
  const void* H = kPartial;
  int64_t ld_h;
  float* dcoef = at<float>(0x52000000);
  int64_t f;
  int dtype = APPNP_F32;
  int K = 3;
  const float* coef = at<float>(0x51000000);
  void* ws = kWs;
  size_t ws_bytes;

  Poly(const appnp_graph* g_, int64_t f_, int K_ = 3)
      : g(g_), ld_x(f_), ld_y(f_), ld_h(f_), f(f_), K(K_),
        ws_bytes(appnp_poly_workspace_bytes(g_, f_, K_, 1)) {}
  int fwd() const {
    return appnp_poly(g, X, ld_x, Y, ld_y, f, dtype, K, coef, ws, ws_bytes, kStream);
  }
  int bwd() const {
    return appnp_poly_bwd(g, X, ld_x, H, ld_h, Y, ld_y, dcoef, f, dtype, K, coef, ws, ws_bytes,
                          kStream);
  }
};

// all four per-iteration entry points: Zin / Zout of the whole-row steps, the split buffers of
// the split-layout ones
struct Step {
  const appnp_graph* g;
  int part = APPNP_PART_ALL;                      // appnp_step, appnp_step_split
  int s_lo = 0, s_hi = 1, mode = APPNP_SHARDS_ONLY;  // the shard variants
  const void* Zin = kZinMain;
  int64_t ld_in;
  const void* H = kH;
  int64_t ld_h;
  void* Zout = kZ;
  int64_t ld_out;
  float* partial = kPartial;
  int64_t ld_partial;
  const float* zin_main = kZinMain;
  const float* zin_rem = kZinRem;
  float* zout_main = kZoutMain;
  float* zout_rem = kZoutRem;
  float* Z = nullptr;  // split-layout steps: null writes the next split buffers
  int64_t ld_z;
  int64_t f;
  int dtype = APPNP_F32;
  int k = 2;
  float alpha = 0.1f, p_drop = 0.0f;
  uint64_t seed = 42;
  void* stream = kStream;

  Step(const appnp_graph* g_, int64_t f_)
      : g(g_), ld_in(f_), ld_h((f_ + 3) / 4 * 4), ld_out(f_), ld_partial((f_ + 3) / 4 * 4),
        ld_z((f_ + 3) / 4 * 4), f(f_) {}
  int step() const {
    return appnp_step(g, part, Zin, ld_in, H, ld_h, Zout, ld_out, partial, ld_partial, f, dtype,
                      k, alpha, p_drop, seed, stream);
  }
  int shards() const {
    return appnp_step_shards(g, s_lo, s_hi, mode, static_cast<const float*>(Zin), ld_in,
                             static_cast<const float*>(H), ld_h, static_cast<float*>(Zout),
                             ld_out, partial, ld_partial, f, k, alpha, p_drop, seed, stream);
  }
  int split() const {
    return appnp_step_split(g, part, zin_main, zin_rem, static_cast<const float*>(H), ld_h,
                            zout_main, zout_rem, Z, ld_z, partial, ld_partial, f, k, alpha,
                            p_drop, seed, stream);
  }
  int split_shards() const {
    return appnp_step_split_shards(g, s_lo, s_hi, mode, zin_main, zin_rem,
                                   static_cast<const float*>(H), ld_h, zout_main, zout_rem, Z,
                                   ld_z, partial, ld_partial, f, k, alpha, p_drop, seed, stream);
  }
};

// the held rows of a row partition with every optional part: the graph of the step cases
constexpr unsigned kPartG = G_ROWS | G_SPLIT | G_SB4 | G_SHARDS;

int spmm(int64_t rows, int64_t cols, const float* B, int64_t ld_b, float* C, int64_t ld_c,
         int64_t f, float p_drop = 0.0f, int tkey = 0, const int32_t* indptr = at<int32_t>(0x70000000)) {
  return appnp_spmm(indptr, at<int32_t>(0x71000000), at<float>(0x72000000), rows, cols, B, ld_b,
                    C, ld_c, f, p_drop, 7, tkey, kStream);
}

int print_launches(const appnp_graph* g) {
  int64_t launches = -1;
  const int rc = appnp_graph_source_block_layout(g, nullptr, nullptr, nullptr, nullptr, &launches);
  printf("rem_launches=%" PRId64 "\n", launches);
  return rc;
}

// the pure queries on one graph
int queries(const appnp_graph* g) {
  const int64_t fs_list[] = {0, 1, 3, 4, 5, 7, 8, 9, 13, 16, 17, 32, 33, 36, 40, 41, 47, 64, 96,
                             100, 128, 200, 256, 257, 260};
  for (int64_t f : fs_list) {
    int64_t fs = -1, r = -1, lfs = -1, lw = -1;
    const int rc_fs = appnp_propagate_split_point(g, f, APPNP_F32, &fs);
    const int rc_r = appnp_propagate_remainder_cols(g, f, APPNP_F32, &r);
    const int rc_l = appnp_split_layout(g, f, &lfs, &lw);
    printf("f=%" PRId64 " ws_f32=%zu ws_bf16=%zu split_point=%d:%" PRId64 " rem_cols=%d:%" PRId64
           " layout=%d:%" PRId64 ":%" PRId64 "\n",
           f, appnp_workspace_bytes(g, f, f, APPNP_F32), appnp_workspace_bytes(g, f, f, APPNP_BF16),
           rc_fs, fs, rc_r, r, rc_l, lfs, lw);
  }
  int64_t fs = -1, r = -1;
  printf("bf16 f=100: split_point=%d:%" PRId64,
         appnp_propagate_split_point(g, 100, APPNP_BF16, &fs), fs);
  printf(" rem_cols=%d:%" PRId64 "\n", appnp_propagate_remainder_cols(g, 100, APPNP_BF16, &r), r);
  int width = -1, value_free = -1, passes = -1;
  int64_t entries = -1, launches = -1, bytes = -1;
  int rc = appnp_graph_source_block_layout(g, &width, &entries, &value_free, &passes, &launches);
  printf("layout rc=%d width=%d entries=%" PRId64 " value_free=%d passes=%d launches=%" PRId64
         "\n", rc, width, entries, value_free, passes, launches);
  rc = appnp_graph_source_blocks(g, &bytes);
  printf("source_blocks rc=%d bytes=%" PRId64 "\n", rc, bytes);
  int64_t n = -1, lo = -1, hi = -1, nnz = -1;
  int mode = -1, sym = -1;
  rc = appnp_graph_info(g, &n, &lo, &hi, &nnz, &mode, &sym);
  printf("info rc=%d n=%" PRId64 " rows=[%" PRId64 ",%" PRId64 ") nnz=%" PRId64
         " mode=%d symmetric=%d\n", rc, n, lo, hi, nnz, mode, sym);
  return APPNP_OK;
}

// run appnp_propagate / _bwd under the kernel timer and print the kinds it recorded
int timed(const Prop& p, bool bwd, int capacity) {
  printf("timer_begin -> %d\n", appnp_kernel_timer_begin(capacity, kStream));
  printf("call -> %d\n", bwd ? p.bwd() : p.fwd());
  float ms[16];
  int kinds[16], n = -1;
  const int rc = appnp_kernel_timer_end(ms, kinds, 16, &n);
  printf("kinds n=%d:", n);
  for (int i = 0; i < n && i < 16 && rc == APPNP_OK; ++i) printf(" %d", kinds[i]);
  printf("\n");
  return rc;
}

const float kNaN = std::numeric_limits<float>::quiet_NaN();
constexpr int64_t kBig = (int64_t)INT32_MAX + 1;

struct Case {
  const char* name;
  int (*run)();
};

#define CASE(name, ...) {name, []() -> int { __VA_ARGS__ }},

const Case kCases[] = {
    // ---- appnp_propagate: whole rows -------------------------------------------------------
    CASE("propagate f32 K=0", Prop p(G(0), 64); p.K = 0; return p.fwd();)
    CASE("propagate f32 K=1", Prop p(G(0), 64); p.K = 1; return p.fwd();)
    CASE("propagate f32 K=1 no ws", Prop p(G(0), 64); p.K = 1; p.ws = nullptr; p.ws_bytes = 0; return p.fwd();)
    CASE("propagate f32 K=1: an unused ws does not count", Prop p(G(0), 64); p.K = 1; p.ws = off(kWs, 8); return p.fwd();)
    CASE("propagate f32 K=2", Prop p(G(0), 64); p.K = 2; return p.fwd();)
    CASE("propagate f32 K=3", Prop p(G(0), 64); p.K = 3; return p.fwd();)
    CASE("propagate bf16 K=0", Prop p(G(0), 64, APPNP_BF16); p.K = 0; return p.fwd();)
    CASE("propagate bf16 K=1", Prop p(G(0), 64, APPNP_BF16); p.K = 1; return p.fwd();)
    CASE("propagate bf16 K=2", Prop p(G(0), 64, APPNP_BF16); p.K = 2; return p.fwd();)
    CASE("propagate bf16 K=3", Prop p(G(0), 64, APPNP_BF16); p.K = 3; return p.fwd();)
    CASE("propagate small graph K=3", Prop p(G(G_SMALL), 64); return p.fwd();)
    CASE("propagate F=7 ld=7", Prop p(G(0), 7); return p.fwd();)
    CASE("propagate F=100", Prop p(G(0), 100); return p.fwd();)
    CASE("propagate F=100 bf16 ld=104", Prop p(G(0), 100, APPNP_BF16); p.ld_h = p.ld_z = 104; return p.fwd();)
    CASE("propagate unaligned ws", Prop p(G(0), 64); p.ws = off(kWs, 16); return p.fwd();)
    CASE("propagate unaligned ws, exact size",
         Prop p(G(0), 64); p.ws = off(kWs, 16); p.ws_bytes = 200000 * 64 * 4 + 240; return p.fwd();)
    CASE("propagate unaligned ws, one byte short",
         Prop p(G(0), 64); p.ws = off(kWs, 16); p.ws_bytes = 200000 * 64 * 4 + 239; return p.fwd();)
    CASE("propagate H not 16-B aligned", Prop p(G(0), 64); p.H = off(kH, 8); return p.fwd();)
    CASE("propagate dropout", Prop p(G(0), 64); p.p_drop = 0.5f; p.seed = 0x1234567; return p.fwd();)
    CASE("propagate dropout tiny p", Prop p(G(0), 64); p.K = 1; p.p_drop = 1e-9f; return p.fwd();)
    CASE("propagate rw graph", Prop p(G(G_RW | G_ASYM | G_TR), 64); return p.fwd();)
    // ---- appnp_propagate: the split layout -------------------------------------------------
    CASE("propagate split F=100 (fs=96)", const appnp_graph* g = G(G_SB4); Prop p(g, 100);
         const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate split F=100 K=2", const appnp_graph* g = G(G_SB4); Prop p(g, 100); p.K = 2;
         const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate split F=3 (fs=0)", const appnp_graph* g = G(G_SB4); Prop p(g, 3);
         p.ld_h = p.ld_z = 4; const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate split W8 F=40", const appnp_graph* g = G(G_SB8); Prop p(g, 40);
         const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate split W16 F=13", const appnp_graph* g = G(G_SB16); Prop p(g, 13);
         p.ld_h = p.ld_z = 16; const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate W16 F=100 keeps whole rows", const appnp_graph* g = G(G_SB16); Prop p(g, 100);
         const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate split unit graph", const appnp_graph* g = G(G_SB4 | G_UNIT); Prop p(g, 100);
         const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate split unit rw graph", const appnp_graph* g = G(G_SB4 | G_UNIT | G_RW);
         Prop p(g, 100); const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate split dropout", const appnp_graph* g = G(G_SB4); Prop p(g, 100);
         p.p_drop = 0.25f; const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate split unaligned ws", const appnp_graph* g = G(G_SB4); Prop p(g, 100);
         p.ws = off(kWs, 48); const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate no split: near_frac > 0.5", const appnp_graph* g = G(G_SB4 | G_NEAR);
         Prop p(g, 100); const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate no split: K=1", const appnp_graph* g = G(G_SB4); Prop p(g, 100); p.K = 1;
         const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate no split: H not 16-B aligned", const appnp_graph* g = G(G_SB4); Prop p(g, 100);
         p.H = off(kH, 4); const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate no split: ld_z not a multiple of 4", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.ld_z = 101; const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate no split: bf16", const appnp_graph* g = G(G_SB4); Prop p(g, 100, APPNP_BF16);
         const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate no split: small graph", const appnp_graph* g = G(G_SB4 | G_SMALL);
         Prop p(g, 100); const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("propagate no split: workspace fits whole rows only", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.ws_bytes = 200000 * 128 * 4; const int rc = p.fwd(); print_launches(g);
         return rc;)
    // two split buffers of [200000, 96] + [200000, 4] fp32: 2 * 80000000 bytes
    CASE("propagate split: workspace fits exactly", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.ws_bytes = 160000000; const int rc = p.fwd(); print_launches(g);
         return rc;)
    CASE("propagate no split: workspace one byte short", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.ws_bytes = 159999999; const int rc = p.fwd(); print_launches(g);
         return rc;)
    CASE("propagate split: unaligned workspace fits exactly", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.ws = off(kWs, 48); p.ws_bytes = 160000000 + 208; const int rc = p.fwd();
         print_launches(g); return rc;)
    CASE("propagate no split: unaligned workspace one byte short", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.ws = off(kWs, 48); p.ws_bytes = 160000000 + 207; const int rc = p.fwd();
         print_launches(g); return rc;)
    // ---- appnp_propagate: rejected arguments -----------------------------------------------
    CASE("propagate: null graph", Prop p(G(0), 64); p.g = nullptr; return p.fwd();)
    CASE("propagate: f < 0", Prop p(G(0), 64); p.f = -1; return p.fwd();)
    CASE("propagate: f > INT32_MAX", Prop p(G(0), 64); p.f = kBig; return p.fwd();)
    CASE("propagate: K < 0", Prop p(G(0), 64); p.K = -1; return p.fwd();)
    CASE("propagate: bad dtype", Prop p(G(0), 64); p.dtype = 2; return p.fwd();)
    CASE("propagate: alpha < 0", Prop p(G(0), 64); p.alpha = -0.1f; return p.fwd();)
    CASE("propagate: alpha > 1", Prop p(G(0), 64); p.alpha = 1.5f; return p.fwd();)
    CASE("propagate: alpha NaN", Prop p(G(0), 64); p.alpha = kNaN; return p.fwd();)
    CASE("propagate: p_drop < 0", Prop p(G(0), 64); p.p_drop = -0.1f; return p.fwd();)
    CASE("propagate: p_drop = 1", Prop p(G(0), 64); p.p_drop = 1.0f; return p.fwd();)
    CASE("propagate: held rows only", Prop p(G(G_ROWS), 64); return p.fwd();)
    CASE("propagate: f = 0 is a no-op", Prop p(G(0), 64); p.f = 0; p.H = nullptr; return p.fwd();)
    CASE("propagate: null H", Prop p(G(0), 64); p.H = nullptr; return p.fwd();)
    CASE("propagate: null Z", Prop p(G(0), 64); p.Z = nullptr; return p.fwd();)
    CASE("propagate: ld_h < f", Prop p(G(0), 64); p.ld_h = 63; return p.fwd();)
    CASE("propagate: ld_z < f", Prop p(G(0), 64); p.ld_z = 63; return p.fwd();)
    CASE("propagate: H == Z", Prop p(G(0), 64); p.Z = kH; return p.fwd();)
    CASE("propagate: K=2 null ws", Prop p(G(0), 64); p.K = 2; p.ws = nullptr; return p.fwd();)
    CASE("propagate: K=2 ws too small", Prop p(G(0), 64); p.K = 2; p.ws_bytes = 200000 * 64 * 4 - 1; return p.fwd();)
    CASE("propagate: K=0 null H", Prop p(G(0), 64); p.K = 0; p.H = nullptr; return p.fwd();)
    CASE("propagate: held rows and null H", Prop p(G(G_ROWS), 64); p.H = nullptr; return p.fwd();)
    // ---- appnp_propagate_bwd ---------------------------------------------------------------
    CASE("propagate_bwd K=0", Prop p(G(0), 64); p.K = 0; return p.bwd();)
    CASE("propagate_bwd K=1", Prop p(G(0), 64); p.K = 1; return p.bwd();)
    CASE("propagate_bwd K=1 no ws", Prop p(G(0), 64); p.K = 1; p.ws = nullptr; p.ws_bytes = 0; return p.bwd();)
    CASE("propagate_bwd K=1: an unused ws that is not 16-B aligned still lowers V", Prop p(G(0), 64); p.K = 1; p.ws = off(kWs, 8); return p.bwd();)
    CASE("propagate_bwd K=2", Prop p(G(0), 64); p.K = 2; return p.bwd();)
    CASE("propagate_bwd K=3", Prop p(G(0), 64); p.K = 3; return p.bwd();)
    CASE("propagate_bwd K=4", Prop p(G(0), 64); p.K = 4; return p.bwd();)
    CASE("propagate_bwd bf16 K=4", Prop p(G(0), 64, APPNP_BF16); p.K = 4; return p.bwd();)
    CASE("propagate_bwd rw graph with transpose K=3", Prop p(G(G_RW | G_ASYM | G_TR), 64); return p.bwd();)
    CASE("propagate_bwd sym graph, asymmetric A, with transpose", Prop p(G(G_ASYM | G_TR), 64); return p.bwd();)
    CASE("propagate_bwd dropout", Prop p(G(0), 64); p.p_drop = 0.5f; return p.bwd();)
    CASE("propagate_bwd unaligned ws K=4", Prop p(G(0), 64); p.K = 4; p.ws = off(kWs, 16); return p.bwd();)
    CASE("propagate_bwd dZ not 16-B aligned", Prop p(G(0), 64); p.H = off(kH, 8); return p.bwd();)
    CASE("propagate_bwd K=2 one buffer suffices", Prop p(G(0), 64); p.K = 2; p.ws_bytes = 200000 * 64 * 4; return p.bwd();)
    CASE("propagate_bwd: K=3 one buffer is too small", Prop p(G(0), 64); p.K = 3; p.ws_bytes = 200000 * 64 * 4; return p.bwd();)
    CASE("propagate_bwd split F=100", const appnp_graph* g = G(G_SB4); Prop p(g, 100); p.K = 4;
         const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd split F=3 (fs=0)", const appnp_graph* g = G(G_SB4); Prop p(g, 3);
         p.ld_h = p.ld_z = 4; const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd split W8 F=40 dropout", const appnp_graph* g = G(G_SB8); Prop p(g, 40);
         p.p_drop = 0.25f; const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd split unit graph", const appnp_graph* g = G(G_SB4 | G_UNIT); Prop p(g, 100);
         const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd split unaligned ws", const appnp_graph* g = G(G_SB4); Prop p(g, 100);
         p.ws = off(kWs, 48); const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd no split: not self-adjoint", const appnp_graph* g = G(G_SB4 | G_RW | G_TR);
         Prop p(g, 100); const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd no split: K=1", const appnp_graph* g = G(G_SB4); Prop p(g, 100); p.K = 1;
         const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd no split: dH not 16-B aligned", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.Z = off(kZ, 4); const int rc = p.bwd(); print_launches(g); return rc;)
    // K=3 whole rows: two buffers of [200000, ld_w] fp32; the split needs 160000000 bytes
    CASE("propagate_bwd split: workspace fits exactly", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.ws_bytes = 160000000; const int rc = p.bwd(); print_launches(g);
         return rc;)
    CASE("propagate_bwd K=2 no split: workspace one byte short", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.K = 2; p.ws_bytes = 159999999; const int rc = p.bwd(); print_launches(g);
         return rc;)
    CASE("propagate_bwd K=2 no split: unaligned workspace one byte short",
         const appnp_graph* g = G(G_SB4); Prop p(g, 100); p.K = 2; p.ws = off(kWs, 48);
         p.ws_bytes = 160000000 + 207; const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd K=2 split: unaligned workspace fits exactly",
         const appnp_graph* g = G(G_SB4); Prop p(g, 100); p.K = 2; p.ws = off(kWs, 48);
         p.ws_bytes = 160000000 + 208; const int rc = p.bwd(); print_launches(g); return rc;)
    CASE("propagate_bwd: no transpose", Prop p(G(G_RW), 64); return p.bwd();)
    CASE("propagate_bwd: sym graph, asymmetric A, no transpose", Prop p(G(G_ASYM), 64); return p.bwd();)
    CASE("propagate_bwd: no transpose and f = 0", Prop p(G(G_RW), 64); p.f = 0; return p.bwd();)
    CASE("propagate_bwd: no transpose and held rows", Prop p(G(G_RW | G_ROWS), 64); return p.bwd();)
    CASE("propagate_bwd: null graph", Prop p(G(0), 64); p.g = nullptr; return p.bwd();)
    CASE("propagate_bwd: K < 0", Prop p(G(0), 64); p.K = -1; return p.bwd();)
    CASE("propagate_bwd: bad dtype", Prop p(G(0), 64); p.dtype = -1; return p.bwd();)
    CASE("propagate_bwd: alpha > 1", Prop p(G(0), 64); p.alpha = 2.0f; return p.bwd();)
    CASE("propagate_bwd: p_drop = 1", Prop p(G(0), 64); p.p_drop = 1.0f; return p.bwd();)
    CASE("propagate_bwd: held rows only", Prop p(G(G_ROWS), 64); return p.bwd();)
    CASE("propagate_bwd: f = 0 is a no-op", Prop p(G(0), 64); p.f = 0; return p.bwd();)
    CASE("propagate_bwd: null dZ", Prop p(G(0), 64); p.H = nullptr; return p.bwd();)
    CASE("propagate_bwd: null dH", Prop p(G(0), 64); p.Z = nullptr; return p.bwd();)
    CASE("propagate_bwd: ld_dz < f", Prop p(G(0), 64); p.ld_h = 63; return p.bwd();)
    CASE("propagate_bwd: ld_dh < f", Prop p(G(0), 64); p.ld_z = 63; return p.bwd();)
    CASE("propagate_bwd: dZ == dH", Prop p(G(0), 64); p.Z = kH; return p.bwd();)
    CASE("propagate_bwd: K=2 null ws", Prop p(G(0), 64); p.K = 2; p.ws = nullptr; return p.bwd();)
    CASE("propagate_bwd: K=2 ws too small", Prop p(G(0), 64); p.K = 2; p.ws_bytes = 200000 * 64 * 4 - 1; return p.bwd();)
    // ---- appnp_solve / appnp_solve_bwd -----------------------------------------------------
    CASE("solve iters=1", Prop p(G(0), 64); p.K = 1; return p.solve();)
    CASE("solve iters=1 no ws", Prop p(G(0), 64); p.K = 1; p.ws = nullptr; p.ws_bytes = 0; return p.solve();)
    CASE("solve iters=1: an unused ws does not count", Prop p(G(0), 64); p.K = 1; p.ws = off(kWs, 8); return p.solve();)
    CASE("solve iters=2", Prop p(G(0), 64); p.K = 2; return p.solve();)
    CASE("solve iters=3", Prop p(G(0), 64); p.K = 3; return p.solve();)
    CASE("solve iters=5", Prop p(G(0), 64); p.K = 5; return p.solve();)
    CASE("solve iters=5 rw", Prop p(G(G_RW | G_TR), 64); p.K = 5; return p.solve();)
    CASE("solve iters=5 F=100 on a graph with a blocked copy", const appnp_graph* g = G(G_SB4);
         Prop p(g, 100); p.K = 5; const int rc = p.solve(); print_launches(g); return rc;)
    CASE("solve iters=3 unaligned ws, alpha=0.25", Prop p(G(0), 64); p.ws = off(kWs, 16); p.alpha = 0.25f; return p.solve();)
    CASE("solve iters=3 H not 16-B aligned", Prop p(G(0), 64); p.H = off(kH, 8); return p.solve();)
    CASE("solve iters=2 one buffer suffices", Prop p(G(0), 64); p.K = 2; p.ws_bytes = 200000 * 64 * 4; return p.solve();)
    CASE("solve: iters=3 one buffer is too small", Prop p(G(0), 64); p.ws_bytes = 200000 * 64 * 4; return p.solve();)
    CASE("solve_bwd iters=1", Prop p(G(0), 64); p.K = 1; return p.solve_bwd();)
    CASE("solve_bwd iters=2", Prop p(G(0), 64); p.K = 2; return p.solve_bwd();)
    CASE("solve_bwd iters=3", Prop p(G(0), 64); p.K = 3; return p.solve_bwd();)
    CASE("solve_bwd iters=5", Prop p(G(0), 64); p.K = 5; return p.solve_bwd();)
    CASE("solve_bwd iters=1 rw with transpose", Prop p(G(G_RW | G_TR), 64); p.K = 1; return p.solve_bwd();)
    CASE("solve_bwd iters=2 rw with transpose", Prop p(G(G_RW | G_TR), 64); p.K = 2; return p.solve_bwd();)
    CASE("solve_bwd iters=3 rw with transpose", Prop p(G(G_RW | G_TR), 64); p.K = 3; return p.solve_bwd();)
    CASE("solve_bwd iters=5 rw with transpose", Prop p(G(G_RW | G_TR), 64); p.K = 5; return p.solve_bwd();)
    CASE("solve_bwd sym with a transpose held: A_hat itself", Prop p(G(G_TR), 64); p.K = 2; return p.solve_bwd();)
    CASE("solve: null graph", Prop p(G(0), 64); p.g = nullptr; return p.solve();)
    CASE("solve: f < 0", Prop p(G(0), 64); p.f = -1; return p.solve();)
    CASE("solve: f > INT32_MAX", Prop p(G(0), 64); p.f = kBig; return p.solve();)
    CASE("solve: iters = 0", Prop p(G(0), 64); p.K = 0; return p.solve();)
    CASE("solve: iters too large", Prop p(G(0), 64); p.K = (1 << 20) + 1; return p.solve();)
    CASE("solve: bad dtype", Prop p(G(0), 64); p.dtype = 7; return p.solve();)
    CASE("solve: alpha = 0", Prop p(G(0), 64); p.alpha = 0.0f; return p.solve();)
    CASE("solve: alpha > 1", Prop p(G(0), 64); p.alpha = 1.5f; return p.solve();)
    CASE("solve: alpha NaN", Prop p(G(0), 64); p.alpha = kNaN; return p.solve();)
    CASE("solve: held rows only", Prop p(G(G_ROWS), 64); return p.solve();)
    CASE("solve: bf16", Prop p(G(0), 64, APPNP_BF16); return p.solve();)
    CASE("solve: asymmetric A", Prop p(G(G_ASYM), 64); return p.solve();)
    CASE("solve: held rows and bf16", Prop p(G(G_ROWS), 64, APPNP_BF16); return p.solve();)
    CASE("solve: rw without transpose runs forward", Prop p(G(G_RW), 64); p.K = 2; return p.solve();)
    CASE("solve_bwd: rw without transpose", Prop p(G(G_RW), 64); return p.solve_bwd();)
    CASE("solve: f = 0 is a no-op", Prop p(G(0), 64); p.f = 0; return p.solve();)
    CASE("solve: null H", Prop p(G(0), 64); p.H = nullptr; return p.solve();)
    CASE("solve: null Z", Prop p(G(0), 64); p.Z = nullptr; return p.solve();)
    CASE("solve: ld_h < f", Prop p(G(0), 64); p.ld_h = 63; return p.solve();)
    CASE("solve: ld_z < f", Prop p(G(0), 64); p.ld_z = 63; return p.solve();)
    CASE("solve: H == Z", Prop p(G(0), 64); p.Z = kH; return p.solve();)
    CASE("solve: iters=2 null ws", Prop p(G(0), 64); p.K = 2; p.ws = nullptr; return p.solve();)
    CASE("solve: iters=2 ws too small", Prop p(G(0), 64); p.K = 2; p.ws_bytes = 200000 * 64 * 4 - 1; return p.solve();)
    CASE("solve_bwd: null dZ", Prop p(G(0), 64); p.H = nullptr; return p.solve_bwd();)
    CASE("solve_bwd: asymmetric A", Prop p(G(G_ASYM | G_TR), 64); return p.solve_bwd();)
    CASE("solve_iterations / solve_weights",
         const float alphas[] = {0.1f, 0.5f, 1.0f, 0.0f, 1.5f}; const float tols[] = {1e-3f, 1e-6f, 0.0f, 1.0f};
         for (float a : alphas) for (float t : tols) {
           int it = -1; const int rc = appnp_solve_iterations(a, t, &it);
           printf("iterations alpha=%a tol=%a -> %d iters=%d\n", (double)a, (double)t, rc, it);
         }
         printf("iterations null out -> %d\n", appnp_solve_iterations(0.1f, 1e-3f, nullptr));
         double w[6];
         for (float a : alphas) {
           for (double& x : w) x = -1.0;
           const int rc = appnp_solve_weights(a, 6, w);
           printf("weights alpha=%a -> %d:", (double)a, rc);
           for (double x : w) printf(" %a", x);
           printf("\n");
         }
         printf("weights null -> %d, iters=0 -> %d, iters too large -> %d\n",
                appnp_solve_weights(0.1f, 6, nullptr), appnp_solve_weights(0.1f, 0, w),
                appnp_solve_weights(0.1f, (1 << 20) + 1, w));
         return APPNP_OK;)
    // ---- the kernel timer and captured plans -----------------------------------------------
    CASE("timer: propagate K=0", Prop p(G(0), 64); p.K = 0; return timed(p, false, 8);)
    CASE("timer: propagate K=3", Prop p(G(0), 64); return timed(p, false, 8);)
    CASE("timer: propagate split K=2", Prop p(G(G_SB4), 100); p.K = 2; return timed(p, false, 8);)
    CASE("timer: propagate split F=3 K=2 (no main launch)", Prop p(G(G_SB4), 3); p.ld_h = p.ld_z = 4; p.K = 2; return timed(p, false, 8);)
    CASE("timer: propagate_bwd K=0", Prop p(G(0), 64); p.K = 0; return timed(p, true, 8);)
    CASE("timer: propagate_bwd K=2", Prop p(G(0), 64); p.K = 2; return timed(p, true, 8);)
    CASE("timer: propagate_bwd split K=2", Prop p(G(G_SB4), 100); p.K = 2; return timed(p, true, 8);)
    CASE("timer: capacity 2, propagate K=3 drops one", Prop p(G(0), 64); return timed(p, false, 2);)
    CASE("timer: solve iters=3", printf("timer_begin -> %d\n", appnp_kernel_timer_begin(4, kStream));
         Prop p(G(0), 64); printf("call -> %d\n", p.solve()); int n = -1;
         const int rc = appnp_kernel_timer_end(nullptr, nullptr, 0, &n); printf("n=%d\n", n); return rc;)
    CASE("timer: every step entry point",
         printf("timer_begin -> %d\n", appnp_kernel_timer_begin(16, kStream));
         const appnp_graph* g = G(kPartG);
         Step s(g, 64);
         printf("step ALL -> %d\n", s.step());
         s.part = APPNP_PART_LOCAL; printf("step LOCAL -> %d\n", s.step());
         s.part = APPNP_PART_REMOTE; printf("step REMOTE -> %d\n", s.step());
         s.mode = APPNP_SHARDS_FIRST; printf("shards FIRST -> %d\n", s.shards());
         s.mode = APPNP_SHARDS_ACC; printf("shards ACC -> %d\n", s.shards());
         s.mode = APPNP_SHARDS_LAST; printf("shards LAST -> %d\n", s.shards());
         s.mode = APPNP_SHARDS_ONLY; printf("shards ONLY -> %d\n", s.shards());
         Step t(g, 100);
         printf("split_copy -> %d\n", appnp_split_copy(g, static_cast<const float*>(kH), 100, 100, kZinMain, kZinRem, kStream));
         t.part = APPNP_PART_LOCAL; printf("split LOCAL -> %d\n", t.split());
         t.part = APPNP_PART_REMOTE; printf("split REMOTE -> %d\n", t.split());
         t.mode = APPNP_SHARDS_FIRST; printf("split_shards FIRST -> %d\n", t.split_shards());
         t.mode = APPNP_SHARDS_LAST; printf("split_shards LAST -> %d\n", t.split_shards());
         float ms[16]; int kinds[16]; int n = -1;
         const int rc = appnp_kernel_timer_end(ms, kinds, 16, &n);
         printf("kinds n=%d:", n); for (int i = 0; i < n && i < 16; ++i) printf(" %d", kinds[i]);
         printf("\n"); return rc;)
    CASE("timer: bad capacity", return appnp_kernel_timer_begin(0, kStream);)
    CASE("timer: end without begin", int n = -1; return appnp_kernel_timer_end(nullptr, nullptr, 0, &n);)
    CASE("plan_create K=3", Prop p(G(0), 64); return p.plan(false);)
    CASE("plan_create split", Prop p(G(G_SB4), 100); p.K = 2; return p.plan(false);)
    CASE("plan_create: null H fails inside the capture", Prop p(G(0), 64); p.H = nullptr; return p.plan(false);)
    CASE("plan_create: null out", Prop p(G(0), 64);
         return appnp_plan_create(p.g, p.H, p.ld_h, p.Z, p.ld_z, p.f, p.dtype, p.K, p.alpha, p.p_drop, p.seed, p.ws, p.ws_bytes, nullptr);)
    CASE("plan_create_solve iters=3", Prop p(G(0), 64); return p.plan(true);)
    CASE("plan_create_solve: null out", Prop p(G(0), 64);
         return appnp_plan_create_solve(p.g, p.H, p.ld_h, p.Z, p.ld_z, p.f, p.dtype, p.K, p.alpha, p.ws, p.ws_bytes, nullptr);)
    CASE("plan_create_solve: null graph", Prop p(G(0), 64); p.g = nullptr; return p.plan(true);)
    CASE("plan_create_solve: iters = 0", Prop p(G(0), 64); p.K = 0; return p.plan(true);)
    CASE("plan_create_solve: alpha = 0", Prop p(G(0), 64); p.alpha = 0.0f; return p.plan(true);)
    CASE("plan_create_solve: bf16", Prop p(G(0), 64, APPNP_BF16); return p.plan(true);)
    CASE("plan_create_solve: asymmetric A", Prop p(G(G_ASYM), 64); return p.plan(true);)
    CASE("plan_create_solve: null H", Prop p(G(0), 64); p.H = nullptr; return p.plan(true);)
    CASE("plan_create_solve: H == Z", Prop p(G(0), 64); p.Z = kH; return p.plan(true);)
    CASE("plan_create_solve: f = 0 captures an empty plan", Prop p(G(0), 64); p.f = 0; return p.plan(true);)
    CASE("plan_create_solve: null ws fails inside the capture", Prop p(G(0), 64); p.ws = nullptr; return p.plan(true);)
    CASE("plan_launch: null plan", return appnp_plan_launch(nullptr, kStream);)
    // ---- appnp_spmm ------------------------------------------------------------------------
    CASE("spmm", return spmm(1000, 2000, kZinMain, 64, kPartial, 64, 64);)
    CASE("spmm dropout, transposed key", return spmm(1000, 2000, kZinMain, 64, kPartial, 64, 64, 0.5f, 1);)
    CASE("spmm F=7 ld=7", return spmm(1000, 2000, kZinMain, 7, kPartial, 7, 7);)
    CASE("spmm C not 16-B aligned", return spmm(1000, 2000, kZinMain, 64, off(kPartial, 8), 64, 64);)
    CASE("spmm cols = 0 needs no B", return spmm(1000, 0, nullptr, 0, kPartial, 64, 64);)
    CASE("spmm: rows < 0", return spmm(-1, 2000, kZinMain, 64, kPartial, 64, 64);)
    CASE("spmm: cols < 0", return spmm(1000, -1, kZinMain, 64, kPartial, 64, 64);)
    CASE("spmm: f < 0", return spmm(1000, 2000, kZinMain, 64, kPartial, 64, -1);)
    CASE("spmm: f > INT32_MAX", return spmm(1000, 2000, kZinMain, kBig, kPartial, kBig, kBig);)
    CASE("spmm: p_drop = 1", return spmm(1000, 2000, kZinMain, 64, kPartial, 64, 64, 1.0f);)
    CASE("spmm: p_drop < 0", return spmm(1000, 2000, kZinMain, 64, kPartial, 64, 64, -0.5f);)
    CASE("spmm: rows = 0 is a no-op", return spmm(0, 2000, nullptr, 0, nullptr, 0, 64);)
    CASE("spmm: f = 0 is a no-op", return spmm(1000, 2000, nullptr, 0, nullptr, 0, 0);)
    CASE("spmm: null indptr", return spmm(1000, 2000, kZinMain, 64, kPartial, 64, 64, 0.0f, 0, nullptr);)
    CASE("spmm: null C", return spmm(1000, 2000, kZinMain, 64, nullptr, 64, 64);)
    CASE("spmm: ld_c < f", return spmm(1000, 2000, kZinMain, 64, kPartial, 63, 64);)
    CASE("spmm: null B", return spmm(1000, 2000, nullptr, 64, kPartial, 64, 64);)
    CASE("spmm: ld_b < f", return spmm(1000, 2000, kZinMain, 63, kPartial, 64, 64);)
    // ---- appnp_step ------------------------------------------------------------------------
    CASE("step ALL f32", Step s(G(kPartG), 64); return s.step();)
    CASE("step ALL bf16", Step s(G(kPartG), 64); s.dtype = APPNP_BF16; return s.step();)
    CASE("step ALL on the whole small graph, dropout", Step s(G(G_SMALL), 64); s.p_drop = 0.5f; s.k = 0; return s.step();)
    CASE("step ALL ignores partial's alignment", Step s(G(kPartG), 64); s.partial = off(kPartial, 4); return s.step();)
    CASE("step ALL: ld_partial never counts", Step s(G(kPartG), 64); s.ld_partial = 63; return s.step();)
    CASE("step LOCAL", Step s(G(kPartG), 64); s.part = APPNP_PART_LOCAL; return s.step();)
    CASE("step LOCAL null H, null partial", Step s(G(kPartG), 64); s.part = APPNP_PART_LOCAL; s.H = nullptr; s.partial = nullptr; return s.step();)
    CASE("step LOCAL with H not 16-B aligned lowers V", Step s(G(kPartG), 64); s.part = APPNP_PART_LOCAL; s.H = off(kH, 8); return s.step();)
    CASE("step LOCAL with partial not 16-B aligned lowers V", Step s(G(kPartG), 64); s.part = APPNP_PART_LOCAL; s.partial = off(kPartial, 4); return s.step();)
    CASE("step LOCAL: ld_h never counts", Step s(G(kPartG), 64); s.part = APPNP_PART_LOCAL; s.ld_h = 3; return s.step();)
    CASE("step REMOTE", Step s(G(kPartG), 64); s.part = APPNP_PART_REMOTE; return s.step();)
    CASE("step REMOTE dropout", Step s(G(kPartG), 64); s.part = APPNP_PART_REMOTE; s.p_drop = 0.5f; return s.step();)
    CASE("step REMOTE ld_partial = 66 lowers V", Step s(G(kPartG), 64); s.part = APPNP_PART_REMOTE; s.ld_partial = 66; return s.step();)
    CASE("step: null graph", Step s(nullptr, 64); return s.step();)
    CASE("step: f < 0", Step s(G(kPartG), 64); s.f = -1; return s.step();)
    CASE("step: bad dtype", Step s(G(kPartG), 64); s.dtype = 2; return s.step();)
    CASE("step: alpha > 1", Step s(G(kPartG), 64); s.alpha = 1.5f; return s.step();)
    CASE("step: p_drop = 1", Step s(G(kPartG), 64); s.p_drop = 1.0f; return s.step();)
    CASE("step: k < 0", Step s(G(kPartG), 64); s.k = -1; return s.step();)
    CASE("step: no held rows is a no-op", Step s(G(G_EMPTY), 64); s.Zin = nullptr; s.part = 9; return s.step();)
    CASE("step: f = 0 is a no-op", Step s(G(kPartG), 64); s.f = 0; s.Zin = nullptr; return s.step();)
    CASE("step: null Zin", Step s(G(kPartG), 64); s.Zin = nullptr; return s.step();)
    CASE("step: null Zout", Step s(G(kPartG), 64); s.Zout = nullptr; return s.step();)
    CASE("step: ld_in < f", Step s(G(kPartG), 64); s.ld_in = 63; return s.step();)
    CASE("step: ld_out < f", Step s(G(kPartG), 64); s.ld_out = 63; return s.step();)
    CASE("step ALL: null H", Step s(G(kPartG), 64); s.H = nullptr; return s.step();)
    CASE("step ALL: ld_h < f", Step s(G(kPartG), 64); s.ld_h = 60; return s.step();)
    CASE("step LOCAL: no halves", Step s(G(G_ROWS), 64); s.part = APPNP_PART_LOCAL; return s.step();)
    CASE("step LOCAL: bf16", Step s(G(kPartG), 64); s.part = APPNP_PART_LOCAL; s.dtype = APPNP_BF16; return s.step();)
    CASE("step REMOTE: null H", Step s(G(kPartG), 64); s.part = APPNP_PART_REMOTE; s.H = nullptr; return s.step();)
    CASE("step REMOTE: ld_h < f", Step s(G(kPartG), 64); s.part = APPNP_PART_REMOTE; s.ld_h = 60; return s.step();)
    CASE("step REMOTE: null partial", Step s(G(kPartG), 64); s.part = APPNP_PART_REMOTE; s.partial = nullptr; return s.step();)
    CASE("step REMOTE: ld_partial < f", Step s(G(kPartG), 64); s.part = APPNP_PART_REMOTE; s.ld_partial = 60; return s.step();)
    CASE("step: part = 3", Step s(G(kPartG), 64); s.part = 3; return s.step();)
    CASE("step: part = -1", Step s(G(kPartG), 64); s.part = -1; return s.step();)
    CASE("step: no halves and part = 3", Step s(G(G_ROWS), 64); s.part = 3; return s.step();)
    CASE("step: no halves and bf16", Step s(G(G_ROWS), 64); s.part = APPNP_PART_LOCAL; s.dtype = APPNP_BF16; return s.step();)
    CASE("step: bf16 and part = 3", Step s(G(kPartG), 64); s.part = 3; s.dtype = APPNP_BF16; return s.step();)
    CASE("step: bf16 REMOTE and null H", Step s(G(kPartG), 64); s.part = APPNP_PART_REMOTE; s.dtype = APPNP_BF16; s.H = nullptr; return s.step();)
    CASE("step: null Zin and no halves", Step s(G(G_ROWS), 64); s.part = APPNP_PART_LOCAL; s.Zin = nullptr; return s.step();)
    // ---- appnp_split_layout / appnp_split_copy ---------------------------------------------
    CASE("split_copy F=100", const appnp_graph* g = G(kPartG);
         return appnp_split_copy(g, static_cast<const float*>(kH), 100, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy F=100 on the whole graph (row_lo = 0)", const appnp_graph* g = G(G_SB4);
         return appnp_split_copy(g, static_cast<const float*>(kH), 104, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy F=3 (fs=0), null main", const appnp_graph* g = G(kPartG);
         return appnp_split_copy(g, static_cast<const float*>(kH), 4, 3, nullptr, kZinRem, kStream);)
    CASE("split_copy unit graph: the scale at the held rows", const appnp_graph* g = G(kPartG | G_UNIT);
         return appnp_split_copy(g, static_cast<const float*>(kH), 100, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy W8 F=40", const appnp_graph* g = G(G_ROWS | G_SB8);
         return appnp_split_copy(g, static_cast<const float*>(kH), 40, 40, kZinMain, kZinRem, kStream);)
    CASE("split_copy: null graph", return appnp_split_copy(nullptr, static_cast<const float*>(kH), 100, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy: f = 0", return appnp_split_copy(G(kPartG), static_cast<const float*>(kH), 100, 0, kZinMain, kZinRem, kStream);)
    CASE("split_copy: no blocked copy", return appnp_split_copy(G(G_ROWS), static_cast<const float*>(kH), 100, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy: F = 47 is not split", return appnp_split_copy(G(kPartG), static_cast<const float*>(kH), 48, 47, kZinMain, kZinRem, kStream);)
    CASE("split_copy: no held rows is a no-op", return appnp_split_copy(G(G_EMPTY | G_SB4), nullptr, 100, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy: null H", return appnp_split_copy(G(kPartG), nullptr, 100, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy: null rem", return appnp_split_copy(G(kPartG), static_cast<const float*>(kH), 100, 100, kZinMain, nullptr, kStream);)
    CASE("split_copy: null main with fs > 0", return appnp_split_copy(G(kPartG), static_cast<const float*>(kH), 100, 100, nullptr, kZinRem, kStream);)
    CASE("split_copy: ld_h < f", return appnp_split_copy(G(kPartG), static_cast<const float*>(kH), 96, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy: ld_h not a multiple of 4", return appnp_split_copy(G(kPartG), static_cast<const float*>(kH), 101, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy: H not 16-B aligned", return appnp_split_copy(G(kPartG), off(static_cast<const float*>(kH), 4), 100, 100, kZinMain, kZinRem, kStream);)
    CASE("split_copy: main not 16-B aligned", return appnp_split_copy(G(kPartG), static_cast<const float*>(kH), 100, 100, off(kZinMain, 8), kZinRem, kStream);)
    CASE("split_copy: rem not 16-B aligned", return appnp_split_copy(G(kPartG), static_cast<const float*>(kH), 100, 100, kZinMain, off(kZinRem, 4), kStream);)
    CASE("split_layout: null graph", return appnp_split_layout(nullptr, 100, nullptr, nullptr);)
    CASE("split_layout: f < 0", return appnp_split_layout(G(kPartG), -1, nullptr, nullptr);)
    CASE("split_layout: null outputs", return appnp_split_layout(G(kPartG), 100, nullptr, nullptr);)
    // ---- appnp_step_split ------------------------------------------------------------------
    CASE("step_split ALL into the next buffers", const appnp_graph* g = G(kPartG); Step s(g, 100);
         const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split ALL into Z", const appnp_graph* g = G(kPartG); Step s(g, 100); s.Z = static_cast<float*>(kZ);
         s.ld_z = 104; const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split LOCAL", const appnp_graph* g = G(kPartG); Step s(g, 100); s.part = APPNP_PART_LOCAL;
         const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split LOCAL with only what it reads", const appnp_graph* g = G(kPartG); Step s(g, 100);
         s.part = APPNP_PART_LOCAL; s.zin_rem = nullptr; s.H = nullptr; s.ld_h = 1; s.zout_main = s.zout_rem = nullptr;
         const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split REMOTE into the next buffers", const appnp_graph* g = G(kPartG); Step s(g, 100);
         s.part = APPNP_PART_REMOTE; const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split REMOTE into Z", const appnp_graph* g = G(kPartG); Step s(g, 100); s.part = APPNP_PART_REMOTE;
         s.Z = static_cast<float*>(kZ); s.zout_main = s.zout_rem = nullptr; const int rc = s.split();
         print_launches(g); return rc;)
    CASE("step_split REMOTE dropout, ld_partial = fs", const appnp_graph* g = G(kPartG); Step s(g, 100);
         s.part = APPNP_PART_REMOTE; s.p_drop = 0.5f; s.ld_partial = 96; const int rc = s.split();
         print_launches(g); return rc;)
    CASE("step_split ALL on the whole graph (row_lo = 0)", const appnp_graph* g = G(G_SB4); Step s(g, 100);
         const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split ALL F=3 (fs=0) into the next buffer", const appnp_graph* g = G(kPartG); Step s(g, 3);
         s.zin_main = nullptr; s.zout_main = nullptr; const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split ALL F=3 (fs=0) into Z", const appnp_graph* g = G(kPartG); Step s(g, 3);
         s.Z = static_cast<float*>(kZ); const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split ALL W8 F=40 into the next buffers", const appnp_graph* g = G(G_ROWS | G_SB8); Step s(g, 40);
         const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split ALL W8 F=40 into Z", const appnp_graph* g = G(G_ROWS | G_SB8); Step s(g, 40);
         s.Z = static_cast<float*>(kZ); const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split ALL unit graph", const appnp_graph* g = G(kPartG | G_UNIT); Step s(g, 100);
         const int rc = s.split(); print_launches(g); return rc;)
    CASE("step_split two finishing steps count two launches", const appnp_graph* g = G(kPartG); Step s(g, 100);
         s.split(); s.part = APPNP_PART_LOCAL; s.split(); s.part = APPNP_PART_REMOTE; const int rc = s.split();
         print_launches(g); return rc;)
    CASE("step_split: null graph", Step s(nullptr, 100); return s.split();)
    CASE("step_split: alpha < 0", Step s(G(kPartG), 100); s.alpha = -1.0f; return s.split();)
    CASE("step_split: p_drop = 1", Step s(G(kPartG), 100); s.p_drop = 1.0f; return s.split();)
    CASE("step_split: f > INT32_MAX", Step s(G(kPartG), 100); s.f = kBig; return s.split();)
    CASE("step_split: k < 0", Step s(G(kPartG), 100); s.k = -1; return s.split();)
    CASE("step_split: part = -1", Step s(G(kPartG), 100); s.part = -1; return s.split();)
    CASE("step_split: part = 3", Step s(G(kPartG), 100); s.part = 3; return s.split();)
    CASE("step_split: no blocked copy", Step s(G(G_ROWS | G_SPLIT), 100); return s.split();)
    CASE("step_split: F = 47 is not split", Step s(G(kPartG), 47); return s.split();)
    CASE("step_split: f = 0 is not split", Step s(G(kPartG), 100); s.f = 0; return s.split();)
    CASE("step_split: no held rows is a no-op", Step s(G(G_EMPTY | G_SB4), 100); s.zin_main = nullptr; return s.split();)
    CASE("step_split LOCAL: no halves", Step s(G(G_ROWS | G_SB4), 100); s.part = APPNP_PART_LOCAL; return s.split();)
    CASE("step_split REMOTE: fs = 0", Step s(G(kPartG), 3); s.part = APPNP_PART_REMOTE; return s.split();)
    CASE("step_split: null zin_main", Step s(G(kPartG), 100); s.zin_main = nullptr; return s.split();)
    CASE("step_split ALL: null zin_rem", Step s(G(kPartG), 100); s.zin_rem = nullptr; return s.split();)
    CASE("step_split REMOTE: null zin_rem", Step s(G(kPartG), 100); s.part = APPNP_PART_REMOTE; s.zin_rem = nullptr; return s.split();)
    CASE("step_split ALL: null H", Step s(G(kPartG), 100); s.H = nullptr; return s.split();)
    CASE("step_split REMOTE: ld_h < f", Step s(G(kPartG), 100); s.part = APPNP_PART_REMOTE; s.ld_h = 96; return s.split();)
    CASE("step_split ALL: null zout_rem", Step s(G(kPartG), 100); s.zout_rem = nullptr; return s.split();)
    CASE("step_split ALL: null zout_main", Step s(G(kPartG), 100); s.zout_main = nullptr; return s.split();)
    CASE("step_split ALL into Z: ld_z < f", Step s(G(kPartG), 100); s.Z = static_cast<float*>(kZ); s.ld_z = 96; return s.split();)
    CASE("step_split LOCAL with Z: ld_z < f", Step s(G(kPartG), 100); s.part = APPNP_PART_LOCAL; s.Z = static_cast<float*>(kZ); s.ld_z = 96; return s.split();)
    CASE("step_split LOCAL: null partial", Step s(G(kPartG), 100); s.part = APPNP_PART_LOCAL; s.partial = nullptr; return s.split();)
    CASE("step_split REMOTE: ld_partial < fs", Step s(G(kPartG), 100); s.part = APPNP_PART_REMOTE; s.ld_partial = 92; return s.split();)
    CASE("step_split ALL: ld_partial never counts", Step s(G(kPartG), 100); s.ld_partial = 3; s.partial = nullptr; return s.split();)
    CASE("step_split ALL: ld_h not a multiple of 4", Step s(G(kPartG), 100); s.ld_h = 101; return s.split();)
    CASE("step_split LOCAL: ld_h never counts", Step s(G(kPartG), 100); s.part = APPNP_PART_LOCAL; s.ld_h = 101; return s.split();)
    CASE("step_split into Z: ld_z not a multiple of 4", Step s(G(kPartG), 100); s.Z = static_cast<float*>(kZ); s.ld_z = 101; return s.split();)
    CASE("step_split into buffers: ld_z never counts", Step s(G(kPartG), 100); s.ld_z = 1; return s.split();)
    CASE("step_split REMOTE: ld_partial not a multiple of 4", Step s(G(kPartG), 100); s.part = APPNP_PART_REMOTE; s.ld_partial = 98; return s.split();)
    CASE("step_split: zin_main not 16-B aligned", Step s(G(kPartG), 100); s.zin_main = off(kZinMain, 4); return s.split();)
    CASE("step_split: zin_rem not 16-B aligned", Step s(G(kPartG), 100); s.zin_rem = off(kZinRem, 4); return s.split();)
    CASE("step_split: H not 16-B aligned", Step s(G(kPartG), 100); s.H = off(kH, 4); return s.split();)
    CASE("step_split LOCAL: H not 16-B aligned", Step s(G(kPartG), 100); s.part = APPNP_PART_LOCAL; s.H = off(kH, 4); return s.split();)
    CASE("step_split: zout_main not 16-B aligned", Step s(G(kPartG), 100); s.zout_main = off(kZoutMain, 8); return s.split();)
    CASE("step_split: zout_rem not 16-B aligned", Step s(G(kPartG), 100); s.zout_rem = off(kZoutRem, 8); return s.split();)
    CASE("step_split: Z not 16-B aligned", Step s(G(kPartG), 100); s.Z = off(static_cast<float*>(kZ), 4); return s.split();)
    CASE("step_split ALL: partial not 16-B aligned", Step s(G(kPartG), 100); s.partial = off(kPartial, 4); return s.split();)
    CASE("step_split: part = 3 and no blocked copy", Step s(G(G_ROWS), 100); s.part = 3; return s.split();)
    CASE("step_split: k < 0 and no blocked copy", Step s(G(G_ROWS), 100); s.k = -1; return s.split();)
    CASE("step_split: no halves and no blocked copy", Step s(G(G_ROWS), 100); s.part = APPNP_PART_LOCAL; return s.split();)
    CASE("step_split: no held rows and no halves", Step s(G(G_EMPTY | G_SB4), 100); s.part = APPNP_PART_LOCAL; return s.split();)
    CASE("step_split LOCAL: no halves and null zin_main", Step s(G(G_ROWS | G_SB4), 100); s.part = APPNP_PART_LOCAL; s.zin_main = nullptr; return s.split();)
    // ---- appnp_graph_shard_offsets / appnp_step_shards -------------------------------------
    CASE("graph_shard_offsets", return appnp_graph_shard_offsets(G(G_ROWS), 3, 66667, kStream);)
    CASE("graph_shard_offsets: null graph", return appnp_graph_shard_offsets(nullptr, 3, 66667, kStream);)
    CASE("step_shards FIRST", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_FIRST; return s.shards();)
    CASE("step_shards FIRST with only what it reads", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_FIRST;
         s.H = nullptr; s.Zout = nullptr; s.ld_h = s.ld_out = 1; return s.shards();)
    CASE("step_shards ACC", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_ACC; s.s_lo = 1; s.s_hi = 2; return s.shards();)
    CASE("step_shards LAST", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_LAST; s.s_lo = 2; s.s_hi = 3; return s.shards();)
    CASE("step_shards ONLY, all three shards", Step s(G(kPartG), 64); s.s_hi = 3; return s.shards();)
    CASE("step_shards ONLY with a null partial", Step s(G(kPartG), 64); s.partial = nullptr; s.ld_partial = 1; return s.shards();)
    CASE("step_shards FIRST, two shards", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_FIRST; s.s_hi = 2; return s.shards();)
    CASE("step_shards LAST, two shards, dropout", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_LAST; s.s_lo = 1; s.s_hi = 3;
         s.p_drop = 0.5f; return s.shards();)
    CASE("step_shards ACC ld_partial = 66 lowers V", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_ACC; s.ld_partial = 66; return s.shards();)
    CASE("step_shards FIRST: H's alignment does not count", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_FIRST; s.H = off(kH, 4); return s.shards();)
    CASE("step_shards ONLY: H not 16-B aligned lowers V", Step s(G(kPartG), 64); s.H = off(kH, 8); return s.shards();)
    CASE("step_shards ONLY: partial's alignment does not count", Step s(G(kPartG), 64); s.partial = off(kPartial, 4); return s.shards();)
    CASE("step_shards: null graph", Step s(nullptr, 64); return s.shards();)
    CASE("step_shards: alpha > 1", Step s(G(kPartG), 64); s.alpha = 1.5f; return s.shards();)
    CASE("step_shards: k < 0", Step s(G(kPartG), 64); s.k = -1; return s.shards();)
    CASE("step_shards: no shard offsets", Step s(G(G_ROWS), 64); return s.shards();)
    CASE("step_shards: s_lo < 0", Step s(G(kPartG), 64); s.s_lo = -1; return s.shards();)
    CASE("step_shards: s_hi > sh_n", Step s(G(kPartG), 64); s.s_hi = 4; return s.shards();)
    CASE("step_shards: empty range", Step s(G(kPartG), 64); s.s_lo = 1; s.s_hi = 1; return s.shards();)
    CASE("step_shards: mode = 4", Step s(G(kPartG), 64); s.mode = 4; return s.shards();)
    CASE("step_shards: mode = -1", Step s(G(kPartG), 64); s.mode = -1; return s.shards();)
    CASE("step_shards: no held rows is a no-op", Step s(G(G_EMPTY | G_SHARDS), 64); s.Zin = nullptr; return s.shards();)
    CASE("step_shards: f = 0 is a no-op", Step s(G(kPartG), 64); s.f = 0; s.Zin = nullptr; return s.shards();)
    CASE("step_shards: null Zin", Step s(G(kPartG), 64); s.Zin = nullptr; return s.shards();)
    CASE("step_shards: ld_in < f", Step s(G(kPartG), 64); s.ld_in = 63; return s.shards();)
    CASE("step_shards FIRST: null partial", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_FIRST; s.partial = nullptr; return s.shards();)
    CASE("step_shards ACC: ld_partial < f", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_ACC; s.ld_partial = 60; return s.shards();)
    CASE("step_shards LAST: null partial", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_LAST; s.partial = nullptr; return s.shards();)
    CASE("step_shards LAST: null Zout", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_LAST; s.Zout = nullptr; return s.shards();)
    CASE("step_shards ONLY: ld_out < f", Step s(G(kPartG), 64); s.ld_out = 63; return s.shards();)
    CASE("step_shards LAST: null H", Step s(G(kPartG), 64); s.mode = APPNP_SHARDS_LAST; s.H = nullptr; return s.shards();)
    CASE("step_shards ONLY: ld_h < f", Step s(G(kPartG), 64); s.ld_h = 60; return s.shards();)
    CASE("step_shards: no shard offsets and mode = 4", Step s(G(G_ROWS), 64); s.mode = 4; return s.shards();)
    CASE("step_shards: no held rows and mode = 4", Step s(G(G_EMPTY | G_SHARDS), 64); s.mode = 4; return s.shards();)
    CASE("step_shards: no held rows and no shard offsets", Step s(G(G_EMPTY), 64); return s.shards();)
    CASE("step_shards: k < 0 and no shard offsets", Step s(G(G_ROWS), 64); s.k = -1; return s.shards();)
    // ---- appnp_step_split_shards -----------------------------------------------------------
    CASE("step_split_shards FIRST", const appnp_graph* g = G(kPartG); Step s(g, 100); s.mode = APPNP_SHARDS_FIRST;
         const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards FIRST with only what it reads", const appnp_graph* g = G(kPartG); Step s(g, 100);
         s.mode = APPNP_SHARDS_FIRST; s.zin_rem = nullptr; s.H = nullptr; s.ld_h = 1; s.zout_main = s.zout_rem = nullptr;
         const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards ACC", const appnp_graph* g = G(kPartG); Step s(g, 100); s.mode = APPNP_SHARDS_ACC;
         s.s_lo = 1; s.s_hi = 2; const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards LAST into the next buffers", const appnp_graph* g = G(kPartG); Step s(g, 100);
         s.mode = APPNP_SHARDS_LAST; s.s_lo = 2; s.s_hi = 3; const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards LAST into Z, two shards, dropout", const appnp_graph* g = G(kPartG); Step s(g, 100);
         s.mode = APPNP_SHARDS_LAST; s.s_lo = 1; s.s_hi = 3; s.Z = static_cast<float*>(kZ); s.p_drop = 0.5f;
         const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards ONLY into the next buffers", const appnp_graph* g = G(kPartG); Step s(g, 100); s.s_hi = 3;
         const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards ONLY into Z with a null partial", const appnp_graph* g = G(kPartG); Step s(g, 100); s.s_hi = 3;
         s.Z = static_cast<float*>(kZ); s.partial = nullptr; s.ld_partial = 1; const int rc = s.split_shards();
         print_launches(g); return rc;)
    CASE("step_split_shards FIRST, two shards", const appnp_graph* g = G(kPartG); Step s(g, 100);
         s.mode = APPNP_SHARDS_FIRST; s.s_hi = 2; const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards ONLY F=3 (fs=0)", const appnp_graph* g = G(kPartG); Step s(g, 3); s.s_hi = 3;
         s.zin_main = nullptr; s.zout_main = nullptr; const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards LAST W8 F=40 into the next buffers", const appnp_graph* g = G(G_ROWS | G_SB8 | G_SHARDS);
         Step s(g, 40); s.mode = APPNP_SHARDS_LAST; const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards LAST unit graph", const appnp_graph* g = G(kPartG | G_UNIT); Step s(g, 100);
         s.mode = APPNP_SHARDS_LAST; const int rc = s.split_shards(); print_launches(g); return rc;)
    CASE("step_split_shards: null graph", Step s(nullptr, 100); return s.split_shards();)
    CASE("step_split_shards: p_drop < 0", Step s(G(kPartG), 100); s.p_drop = -0.5f; return s.split_shards();)
    CASE("step_split_shards: k < 0", Step s(G(kPartG), 100); s.k = -1; return s.split_shards();)
    CASE("step_split_shards: no blocked copy", Step s(G(G_ROWS | G_SHARDS), 100); return s.split_shards();)
    CASE("step_split_shards: F = 47 is not split", Step s(G(kPartG), 47); return s.split_shards();)
    CASE("step_split_shards: no shard offsets", Step s(G(G_ROWS | G_SB4), 100); return s.split_shards();)
    CASE("step_split_shards: s_lo < 0", Step s(G(kPartG), 100); s.s_lo = -1; return s.split_shards();)
    CASE("step_split_shards: s_hi > sh_n", Step s(G(kPartG), 100); s.s_hi = 4; return s.split_shards();)
    CASE("step_split_shards: empty range", Step s(G(kPartG), 100); s.s_lo = 2; s.s_hi = 1; return s.split_shards();)
    CASE("step_split_shards: mode = 4", Step s(G(kPartG), 100); s.mode = 4; return s.split_shards();)
    CASE("step_split_shards: no held rows is a no-op", Step s(G(G_EMPTY | G_SB4 | G_SHARDS), 100); s.zin_main = nullptr; return s.split_shards();)
    CASE("step_split_shards FIRST: fs = 0", Step s(G(kPartG), 3); s.mode = APPNP_SHARDS_FIRST; return s.split_shards();)
    CASE("step_split_shards LAST: fs = 0", Step s(G(kPartG), 3); s.mode = APPNP_SHARDS_LAST; return s.split_shards();)
    CASE("step_split_shards: null zin_main", Step s(G(kPartG), 100); s.zin_main = nullptr; return s.split_shards();)
    CASE("step_split_shards ONLY: null zin_rem", Step s(G(kPartG), 100); s.zin_rem = nullptr; return s.split_shards();)
    CASE("step_split_shards LAST: null H", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_LAST; s.H = nullptr; return s.split_shards();)
    CASE("step_split_shards ONLY: ld_h < f", Step s(G(kPartG), 100); s.ld_h = 96; return s.split_shards();)
    CASE("step_split_shards ONLY: null zout_rem", Step s(G(kPartG), 100); s.zout_rem = nullptr; return s.split_shards();)
    CASE("step_split_shards LAST: null zout_main", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_LAST; s.zout_main = nullptr; return s.split_shards();)
    CASE("step_split_shards ONLY into Z: ld_z < f", Step s(G(kPartG), 100); s.Z = static_cast<float*>(kZ); s.ld_z = 96; return s.split_shards();)
    CASE("step_split_shards FIRST with Z: ld_z < f", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_FIRST; s.Z = static_cast<float*>(kZ); s.ld_z = 96; return s.split_shards();)
    CASE("step_split_shards FIRST: null partial", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_FIRST; s.partial = nullptr; return s.split_shards();)
    CASE("step_split_shards ACC: ld_partial < fs", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_ACC; s.ld_partial = 92; return s.split_shards();)
    CASE("step_split_shards LAST: null partial", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_LAST; s.partial = nullptr; return s.split_shards();)
    CASE("step_split_shards ONLY: ld_h not a multiple of 4", Step s(G(kPartG), 100); s.ld_h = 101; return s.split_shards();)
    CASE("step_split_shards FIRST: ld_h never counts", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_FIRST; s.ld_h = 101; return s.split_shards();)
    CASE("step_split_shards into Z: ld_z not a multiple of 4", Step s(G(kPartG), 100); s.Z = static_cast<float*>(kZ); s.ld_z = 101; return s.split_shards();)
    CASE("step_split_shards ACC: ld_partial not a multiple of 4", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_ACC; s.ld_partial = 98; return s.split_shards();)
    CASE("step_split_shards ONLY: ld_partial never counts", Step s(G(kPartG), 100); s.ld_partial = 98; return s.split_shards();)
    CASE("step_split_shards: zin_main not 16-B aligned", Step s(G(kPartG), 100); s.zin_main = off(kZinMain, 4); return s.split_shards();)
    CASE("step_split_shards FIRST: zin_rem not 16-B aligned", Step s(G(kPartG), 100); s.mode = APPNP_SHARDS_FIRST; s.zin_rem = off(kZinRem, 4); return s.split_shards();)
    CASE("step_split_shards: H not 16-B aligned", Step s(G(kPartG), 100); s.H = off(kH, 4); return s.split_shards();)
    CASE("step_split_shards: zout_main not 16-B aligned", Step s(G(kPartG), 100); s.zout_main = off(kZoutMain, 8); return s.split_shards();)
    CASE("step_split_shards: zout_rem not 16-B aligned", Step s(G(kPartG), 100); s.zout_rem = off(kZoutRem, 8); return s.split_shards();)
    CASE("step_split_shards: Z not 16-B aligned", Step s(G(kPartG), 100); s.Z = off(static_cast<float*>(kZ), 4); return s.split_shards();)
    CASE("step_split_shards ONLY: partial not 16-B aligned", Step s(G(kPartG), 100); s.partial = off(kPartial, 4); return s.split_shards();)
    CASE("step_split_shards: no blocked copy and no shard offsets", Step s(G(G_ROWS), 100); return s.split_shards();)
    CASE("step_split_shards: no shard offsets and FIRST with fs = 0", Step s(G(G_ROWS | G_SB4), 3); s.mode = APPNP_SHARDS_FIRST; return s.split_shards();)
    CASE("step_split_shards: k < 0 and no blocked copy", Step s(G(G_ROWS | G_SHARDS), 100); s.k = -1; return s.split_shards();)
    CASE("step_split_shards: no held rows and mode = 4", Step s(G(G_EMPTY | G_SB4 | G_SHARDS), 100); s.mode = 4; return s.split_shards();)
    CASE("step_split_shards: no held rows and FIRST with fs = 0", Step s(G(G_EMPTY | G_SB4 | G_SHARDS), 3); s.mode = APPNP_SHARDS_FIRST; return s.split_shards();)
    // ---- pure queries ----------------------------------------------------------------------
    CASE("queries: plain graph", return queries(G(0));)
    CASE("queries: small graph with a blocked copy", return queries(G(G_SMALL | G_SB4));)
    CASE("queries: W4 copy", return queries(G(G_SB4));)
    CASE("queries: W8 copy", return queries(G(G_SB8));)
    CASE("queries: W16 copy", return queries(G(G_SB16));)
    CASE("queries: unit W4 copy", return queries(G(G_SB4 | G_UNIT));)
    CASE("queries: unit rw W4 copy", return queries(G(G_SB4 | G_UNIT | G_RW));)
    CASE("queries: W4 copy, gather locality", return queries(G(G_SB4 | G_NEAR));)
    CASE("queries: held rows, W4 copy", return queries(G(kPartG));)
    CASE("queries: rejected arguments",
         int64_t v = -1; const appnp_graph* g = G(G_SB4);
         printf("workspace_bytes null graph=%zu f<0=%zu bad dtype=%zu\n", appnp_workspace_bytes(nullptr, 64, 64, 0),
                appnp_workspace_bytes(g, -1, 64, 0), appnp_workspace_bytes(g, 64, 64, 2));
         printf("split_point null graph=%d null out=%d f<0=%d bad dtype=%d\n", appnp_propagate_split_point(nullptr, 100, 0, &v),
                appnp_propagate_split_point(g, 100, 0, nullptr), appnp_propagate_split_point(g, -1, 0, &v),
                appnp_propagate_split_point(g, 100, 2, &v));
         printf("remainder_cols null graph=%d null out=%d f<0=%d bad dtype=%d\n", appnp_propagate_remainder_cols(nullptr, 100, 0, &v),
                appnp_propagate_remainder_cols(g, 100, 0, nullptr), appnp_propagate_remainder_cols(g, -1, 0, &v),
                appnp_propagate_remainder_cols(g, 100, 2, &v));
         printf("source_block_layout null graph=%d source_blocks null graph=%d null out=%d\n",
                appnp_graph_source_block_layout(nullptr, nullptr, nullptr, nullptr, nullptr, &v),
                appnp_graph_source_blocks(nullptr, &v), appnp_graph_source_blocks(g, nullptr));
         const double* d = nullptr; const int32_t* rp = nullptr; const int32_t* c = nullptr; const float* x = nullptr;
         printf("graph_info null=%d graph_csr null=%d graph_dinv null graph=%d null out=%d\n",
                appnp_graph_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                appnp_graph_csr(nullptr, &rp, &c, &x), appnp_graph_dinv(nullptr, &d), appnp_graph_dinv(g, nullptr));
         int rc = appnp_graph_csr(g, &rp, &c, &x);
         printf("graph_csr -> %d %#llx %#llx %#llx\n", rc, X(rp), X(c), X(x));
         rc = appnp_graph_dinv(g, &d);
         printf("graph_dinv -> %d %#llx\n", rc, X(d));
         printf("abi=%d strerror: %s | %s | %s | %s | %s | %s | %s\n", appnp_abi_version(), appnp_strerror(0),
                appnp_strerror(-5), appnp_strerror(-12), appnp_strerror(-22), appnp_strerror(-34),
                appnp_strerror(-95), appnp_strerror(1));
         printf("tuning_overrides='%s' tuning_names='%s'\n", appnp_tuning_overrides(), appnp_tuning_names());
         return APPNP_OK;)
    CASE("graph_copy_csr", return appnp_graph_copy_csr(G(kPartG), at<int32_t>(0x80000000), at<int32_t>(0x81000000),
                                                       at<float>(0x82000000), at<double>(0x83000000), kStream);)
    CASE("graph_copy_csr: only dinv", return appnp_graph_copy_csr(G(kPartG), nullptr, nullptr, nullptr, at<double>(0x83000000), kStream);)
    CASE("graph_copy_csr: null graph", return appnp_graph_copy_csr(nullptr, nullptr, nullptr, nullptr, nullptr, kStream);)
    // ---- appnp_graph_create(_rows): which builders run --------------------------------------
    CASE("graph_create sym", appnp_graph* g = nullptr;
         const int rc = appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), at<float>(0x72000000), 1000, 8000,
                                           APPNP_NORM_SYM, kStream, &g);
         appnp_graph_destroy(g); return rc;)
    CASE("graph_create rw, transpose, W8 copy", appnp_graph* g = nullptr;
         const int rc = appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, 1000, 8000,
                                           APPNP_NORM_RW | APPNP_GRAPH_TRANSPOSE | APPNP_GRAPH_SB_W8, kStream, &g);
         appnp_graph_destroy(g); return rc;)
    CASE("graph_create W16 copy that does not fit stays whole rows", appnp_graph* g = nullptr; appnp::g_build_rc = APPNP_ENOMEM;
         const int rc = appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, 1000, 8000,
                                           APPNP_NORM_SYM | APPNP_GRAPH_SB_W16 | APPNP_GRAPH_SOURCE_BLOCKS, kStream, &g);
         appnp::g_build_rc = APPNP_OK; appnp_graph_destroy(g); return rc;)
    CASE("graph_create: a device error in the blocked copy fails", appnp_graph* g = at<appnp_graph>(0xbad0); appnp::g_build_rc = APPNP_EDEVICE;
         const int rc = appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, 1000, 8000,
                                           APPNP_GRAPH_SOURCE_BLOCKS, kStream, &g);
         appnp::g_build_rc = APPNP_OK; printf("g=%#llx\n", X(g)); return rc;)
    CASE("graph_create_rows held rows with halves", appnp_graph* g = nullptr;
         const int rc = appnp_graph_create_rows(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, 1000, 8000,
                                                APPNP_NORM_SYM | APPNP_GRAPH_SOURCE_BLOCKS, 250, 750, 1, kStream, &g);
         appnp_graph_destroy(g); return rc;)
    CASE("graph_create: null out", return appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, 1000, 8000, 0, kStream, nullptr);)
    CASE("graph_create: n < 0", appnp_graph* g = nullptr; return appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, -1, 8000, 0, kStream, &g);)
    CASE("graph_create: n > INT32_MAX", appnp_graph* g = nullptr; return appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, kBig, 8000, 0, kStream, &g);)
    CASE("graph_create: nnz < 0 and n > INT32_MAX", appnp_graph* g = nullptr; return appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, kBig, -1, 0, kStream, &g);)
    CASE("graph_create: bad mode", appnp_graph* g = nullptr; return appnp_graph_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, 1000, 8000, 2, kStream, &g);)
    CASE("graph_create_rows: row_hi > n", appnp_graph* g = nullptr; return appnp_graph_create_rows(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, 1000, 8000, 0, 0, 1001, 0, kStream, &g);)
    CASE("graph_create_rows: transpose of held rows", appnp_graph* g = nullptr; return appnp_graph_create_rows(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, 1000, 8000, APPNP_GRAPH_TRANSPOSE, 0, 500, 0, kStream, &g);)
    CASE("graph_create: null indptr", appnp_graph* g = nullptr; return appnp_graph_create(nullptr, at<int32_t>(0x71000000), nullptr, 1000, 8000, 0, kStream, &g);)
    CASE("graph_create: null indices", appnp_graph* g = nullptr; return appnp_graph_create(at<int32_t>(0x70000000), nullptr, nullptr, 1000, 8000, 0, kStream, &g);)
    // ---- appnp_poly / appnp_poly_bwd -------------------------------------------------------
    CASE("poly K=0", Poly p(G(0), 64, 0); return p.fwd();)
    CASE("poly K=1", Poly p(G(0), 64, 1); return p.fwd();)
    CASE("poly K=1 no ws", Poly p(G(0), 64, 1); p.ws = nullptr; p.ws_bytes = 0; return p.fwd();)
    CASE("poly K=2", Poly p(G(0), 64, 2); return p.fwd();)
    CASE("poly K=3", Poly p(G(0), 64); return p.fwd();)
    CASE("poly K=5", Poly p(G(0), 64, 5); return p.fwd();)
    CASE("poly F=100 ld=104", Poly p(G(0), 100); p.ld_x = p.ld_y = 104; return p.fwd();)
    CASE("poly F=7 on a small graph", Poly p(G(G_SMALL), 7); return p.fwd();)
    CASE("poly rw graph, no transpose", Poly p(G(G_RW | G_ASYM), 64); return p.fwd();)
    CASE("poly F=100 on a graph with a blocked copy", const appnp_graph* g = G(G_SB4);
         Poly p(g, 100); const int rc = p.fwd(); print_launches(g); return rc;)
    CASE("poly unaligned ws", Poly p(G(0), 64); p.ws = off(kWs, 16); return p.fwd();)
    CASE("poly H not 16-B aligned", Poly p(G(0), 64); p.X = off(kH, 8); return p.fwd();)
    // two buffers of [200000, 64] fp32
    CASE("poly unaligned ws, exact size", Poly p(G(0), 64); p.ws = off(kWs, 16); p.ws_bytes = 102400000 + 240; return p.fwd();)
    CASE("poly: unaligned ws, one byte short", Poly p(G(0), 64); p.ws = off(kWs, 16); p.ws_bytes = 102400000 + 239; return p.fwd();)
    CASE("poly K=2 one buffer suffices", Poly p(G(0), 64, 2); p.ws_bytes = 51200000; return p.fwd();)
    CASE("poly: K=3 one buffer is too small", Poly p(G(0), 64); p.ws_bytes = 51200000; return p.fwd();)
    CASE("poly_bwd K=0", Poly p(G(0), 64, 0); return p.bwd();)
    CASE("poly_bwd K=0 without dcoef needs no ws", Poly p(G(0), 64, 0); p.dcoef = nullptr; p.ws = nullptr; p.ws_bytes = 0; return p.bwd();)
    CASE("poly_bwd K=1", Poly p(G(0), 64, 1); return p.bwd();)
    CASE("poly_bwd K=2", Poly p(G(0), 64, 2); return p.bwd();)
    CASE("poly_bwd K=3", Poly p(G(0), 64); return p.bwd();)
    CASE("poly_bwd K=4 F=100", Poly p(G(0), 100, 4); return p.bwd();)
    CASE("poly_bwd K=3 without dcoef: H is not read", Poly p(G(0), 64); p.dcoef = nullptr; p.ld_h = 63; return p.bwd();)
    CASE("poly_bwd H with its own leading dimension", Poly p(G(0), 64); p.ld_h = 66; return p.bwd();)
    CASE("poly_bwd rw graph with transpose", Poly p(G(G_RW | G_TR), 64); return p.bwd();)
    CASE("poly_bwd sym graph, asymmetric A, with transpose", Poly p(G(G_ASYM | G_TR), 64); return p.bwd();)
    CASE("poly_bwd sym with a transpose held: A_hat itself", Poly p(G(G_TR), 64, 2); return p.bwd();)
    CASE("poly_bwd unaligned ws", Poly p(G(0), 64); p.ws = off(kWs, 48); return p.bwd();)
    // two buffers and one slab of partial dots [200000] fp32
    CASE("poly_bwd ws exact size", Poly p(G(0), 64); p.ws_bytes = 102400000 + 800000; return p.bwd();)
    CASE("poly_bwd: ws one byte short", Poly p(G(0), 64); p.ws_bytes = 102400000 + 800000 - 1; return p.bwd();)
    CASE("poly_bwd: K=0 with dcoef and no ws", Poly p(G(0), 64, 0); p.ws = nullptr; return p.bwd();)
    CASE("poly: null graph", Poly p(G(0), 64); p.g = nullptr; return p.fwd();)
    CASE("poly: f < 0", Poly p(G(0), 64); p.f = -1; return p.fwd();)
    CASE("poly: f > INT32_MAX", Poly p(G(0), 64); p.f = kBig; return p.fwd();)
    CASE("poly: K < 0", Poly p(G(0), 64); p.K = -1; return p.fwd();)
    CASE("poly: K too large", Poly p(G(0), 64); p.K = APPNP_POLY_MAX_K + 1; return p.fwd();)
    CASE("poly: bad dtype", Poly p(G(0), 64); p.dtype = 7; return p.fwd();)
    CASE("poly: bf16", Poly p(G(0), 64); p.dtype = APPNP_BF16; return p.fwd();)
    CASE("poly: held rows only", Poly p(G(G_ROWS), 64); return p.fwd();)
    CASE("poly: held rows and bf16", Poly p(G(G_ROWS), 64); p.dtype = APPNP_BF16; return p.fwd();)
    CASE("poly: f = 0 is a no-op", Poly p(G(0), 64); p.f = 0; p.X = nullptr; p.coef = nullptr; return p.fwd();)
    CASE("poly: null H", Poly p(G(0), 64); p.X = nullptr; return p.fwd();)
    CASE("poly: null Z", Poly p(G(0), 64); p.Y = nullptr; return p.fwd();)
    CASE("poly: null coef", Poly p(G(0), 64); p.coef = nullptr; return p.fwd();)
    CASE("poly: ld_h < f", Poly p(G(0), 64); p.ld_x = 63; return p.fwd();)
    CASE("poly: H == Z", Poly p(G(0), 64); p.Y = kH; return p.fwd();)
    CASE("poly: K=2 null ws", Poly p(G(0), 64, 2); p.ws = nullptr; return p.fwd();)
    CASE("poly_bwd: rw without transpose", Poly p(G(G_RW), 64); return p.bwd();)
    CASE("poly_bwd: sym graph, asymmetric A, no transpose", Poly p(G(G_ASYM), 64); return p.bwd();)
    CASE("poly_bwd: no transpose and f = 0", Poly p(G(G_RW), 64); p.f = 0; return p.bwd();)
    CASE("poly_bwd: no transpose and held rows", Poly p(G(G_RW | G_ROWS), 64); return p.bwd();)
    CASE("poly_bwd: bf16", Poly p(G(0), 64); p.dtype = APPNP_BF16; return p.bwd();)
    CASE("poly_bwd: null coef", Poly p(G(0), 64); p.coef = nullptr; return p.bwd();)
    CASE("poly_bwd: dZ == dH", Poly p(G(0), 64); p.Y = kH; return p.bwd();)
    CASE("poly_bwd: dcoef and null H", Poly p(G(0), 64); p.H = nullptr; return p.bwd();)
    CASE("poly_bwd: dcoef and ld_h < f", Poly p(G(0), 64); p.ld_h = 63; return p.bwd();)
    CASE("poly_bwd: dcoef and H == dH", Poly p(G(0), 64); p.H = kZ; return p.bwd();)
    CASE("poly_workspace_bytes",
         const appnp_graph* g = G(0); const appnp_graph* rows = G(G_ROWS); const appnp_graph* none = G(G_EMPTY);
         const int64_t fs_list[] = {-1, 0, 1, 7, 32, 33, 64, 100, 260, kBig};
         const int ks[] = {-1, 0, 1, 2, 3, 10, APPNP_POLY_MAX_K, APPNP_POLY_MAX_K + 1};
         for (int64_t f : fs_list) for (int k : ks)
           printf("f=%" PRId64 " K=%d: %zu %zu held rows %zu %zu\n", f, k, appnp_poly_workspace_bytes(g, f, k, 0),
                  appnp_poly_workspace_bytes(g, f, k, 1), appnp_poly_workspace_bytes(rows, f, k, 0),
                  appnp_poly_workspace_bytes(rows, f, k, 1));
         printf("null graph %zu, no rows %zu\n", appnp_poly_workspace_bytes(nullptr, 64, 3, 1),
                appnp_poly_workspace_bytes(none, 64, 3, 1));
         return APPNP_OK;)
};

}  // namespace

int main() {
  for (const Case& c : kCases) {
    printf("# %s\n", c.name);
    g_next_handle = 0xe0000000u;
    const int rc = c.run();
    printf("-> %d\n", rc);
    g_graphs.clear();
  }
  return 0;
}

#endif  // TRACE_STANDINS_ONLY
