// appnp_internal.h -- host-side internals shared by the translation units of libppnp_amd.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "appnp_device.h"
#include "../../include/ppnp_amd.h"

struct appnp_graph {
  int64_t n = 0;         // global node count
  int64_t row_lo = 0;    // held rows [row_lo, row_hi)
  int64_t row_hi = 0;
  int64_t nnz_hat = 0;   // nnz of the held A_hat rows
  int64_t nnz_local = 0, nnz_remote = 0;
  int mode = 0;          // APPNP_NORM_SYM / APPNP_NORM_RW
  int symmetric = 0;     // A's pattern and weights are symmetric
  int unit = 0;          // every entry of A+I is 1 (unweighted A, no self loops): A_hat is
                         // dl_i * dr_j with per-row scales (sym: dinv, dinv; rw: dinv, 1)
  int split = 0;         // local/remote CSRs present
  int device = 0;
  int32_t* row_ptr = nullptr;   // [rows+1]
  int32_t* col = nullptr;       // [nnz_hat]
  float* val = nullptr;         // [nnz_hat]
  int32_t* lrow_ptr = nullptr;  // local-column CSR (split only)
  int32_t* lcol = nullptr;
  float* lval = nullptr;
  int32_t* rrow_ptr = nullptr;  // remote-column CSR (split only)
  int32_t* rcol = nullptr;
  float* rval = nullptr;
  double* dinv = nullptr;       // [n] 1/sqrt(D) (sym) or 1/D (rw), fp64
  int32_t* heavy = nullptr;     // rows with > kHeavyRow entries (ascending)
  int64_t n_heavy = 0;
  int32_t* t_heavy = nullptr;   // the same for A_hat^T
  int64_t t_n_heavy = 0;
  int32_t* hub = nullptr;       // rows with > kHubRow entries: dispatched first (wide kernels)
  int64_t n_hub = 0;
  int32_t* t_hub = nullptr;
  int64_t t_n_hub = 0;
  int32_t* t_row_ptr = nullptr; // A_hat^T (APPNP_GRAPH_TRANSPOSE, when A_hat is not symmetric)
  int32_t* t_col = nullptr;
  float* t_val = nullptr;
  // A_hat regrouped for the persistent remainder pass (APPNP_GRAPH_SOURCE_BLOCKS,
  // appnp_blocks.hip): segment (group, source block) holds the entries of one wave's group of
  // rows whose column lies in that block, sorted by (row, column), padded to 64 entries
  int32_t* rb_off = nullptr;    // [rb_passes * rb_slots * rb_nb + 1] segment starts
  uint32_t* rb_ent = nullptr;   // [rb_total] (row in group << kRemColBits) | column in block
  float* rb_val = nullptr;      // [rb_total]; null for a unit graph (values from rb_dl/rb_dr)
  float* rb_dl = nullptr;       // unit graph: [n] fp32 dinv, the row scale of A_hat
  float* rb_dr = nullptr;       // unit graph, sym: [n] fp32 dinv, the column scale (rw: null)
  int32_t* rb_cblk = nullptr;   // [rb_total / 64] source block of each chunk of 64 entries
  int64_t rb_total = 0;         // entries including the padding
  int32_t rb_nb = 0;            // source blocks of 2^rb_br_log2 rows
  int32_t rb_br_log2 = 0;
  int32_t rb_grid = 0;          // workgroups of the pass (one per CU)
  int32_t rb_slots = 0;         // groups per pass = rb_grid * kRemWaves
  int32_t rb_rg = 0;            // rows per group
  int32_t rb_passes = 0;
  int32_t rb_lpe = 0;           // lanes per entry of the pass: remainder rows of 4 rb_lpe columns
  // shard offsets of the held rows (appnp_graph_shard_offsets): entries of held row i with a
  // column in shard s ([s sh_rows, (s+1) sh_rows)) are sh_off[s rows + i] .. sh_off[(s+1) rows + i]
  int32_t* sh_off = nullptr;    // [(sh_n + 1) * rows]
  int32_t sh_n = 0;
  int64_t sh_rows = 0;
  double near_frac = 0.0;       // off-diagonal entries within kNearRows of their row / nnz
  // remainder-pass launches enqueued on this graph (appnp_graph_source_block_layout): the path
  // witness the tests read
  mutable std::atomic<int64_t> rem_launches{0};
};

struct appnp_csr;

namespace appnp {

// appnp_graph.hip
int graph_build(const int32_t* indptr, const int32_t* indices, const float* vals, int64_t n,
                int64_t nnz, int mode, int64_t row_lo, int64_t row_hi, int split,
                hipStream_t s, appnp_graph* g);
void graph_free(appnp_graph* g);
void graph_free_source_blocks(appnp_graph* g);
int graph_build_shard_offsets(appnp_graph* g, int nshards, int64_t shard_rows, hipStream_t s);
int graph_build_transpose(appnp_graph* g, hipStream_t s);
int build_heavy(const int32_t* rp, int64_t rows, int32_t thr, hipStream_t s, int32_t** out,
                int64_t* n_out);
int64_t scan_partials(int64_t rows);

// appnp_ingest.hip
int csr_transpose(const int32_t* indptr, const int32_t* indices, const float* vals, int64_t rows,
                  int64_t cols, int64_t nnz, hipStream_t s, appnp_csr* out);
void csr_free(appnp_csr* c);
hipError_t exclusive_scan(const int32_t* cnt, int64_t rows, int32_t* out, int64_t* d_bsum,
                          int64_t* d_total, hipStream_t s);

// appnp_blocks.hip
// lpe: lanes per entry of the remainder pass (1, 2, 4: remainder rows of 4, 8, 16 columns)
// a_indptr / a_indices / a_nnz: the whole graph's A (the row partition's gather-locality
// measure is taken over all of it, so every rank decides the same split)
int graph_build_source_blocks(appnp_graph* g, int lpe, const int32_t* a_indptr,
                              const int32_t* a_indices, int64_t a_nnz, hipStream_t s);
// to_rem: out is the next remainder buffer (a unit graph stores dr o y there), not Z / dH
hipError_t launch_remainder(const appnp_graph* g, const StepArgs& a, int epi,
                            const float* z_rem, const float* h_rem, int64_t ld_h, float* out,
                            int64_t ld_out, int nv, bool to_rem, hipStream_t s);
// rem_scale (nullable): per-row factor of the remainder part (remainder_scale(g))
// rw: floats per remainder row (4 rb_lpe)
hipError_t launch_split_copy(const float* h, int64_t ld_h, int64_t n, int64_t f, int64_t fs,
                             int64_t rw, float* main, float* rem, const float* rem_scale,
                             hipStream_t s);
// the factor the remainder buffers carry: dr for a value-free (unit) layout, else none
inline const float* remainder_scale(const appnp_graph* g) {
  return g->rb_val ? nullptr : g->rb_dr;
}

// appnp_spmm.hip
int pick_vec(int dtype, int64_t f, const int64_t* lds, int n_ld, const void* const* ptrs,
             int n_ptr);
hipError_t launch_step(int dtype, int epi, int V, const StepArgs& a, hipStream_t s);
// launch_step that also reports (slabs_out, nullable) the column slabs it covers the rows with
// (gridDim.y): the leading extent of StepArgs::dots
hipError_t launch_step_slabs(int dtype, int epi, int V, const StepArgs& a, hipStream_t s,
                             int64_t* slabs_out);
// appnp_poly: dst = (*coef) * src by rows and, with dots, dots[i] = <src[i], h[i]>; *out = the
// sum of part[0 .. count) in a fixed order; the most slabs launch_step takes for f features
hipError_t launch_poly_rows(const float* src, int64_t ld_src, float* dst, int64_t ld_dst,
                            const float* h, int64_t ld_h, float* dots, int64_t n, int64_t f,
                            const float* coef, hipStream_t s);
hipError_t launch_poly_reduce(const float* part, int64_t count, float* out, hipStream_t s);
int64_t poly_max_slabs(int64_t f);
hipError_t launch_scale_rows(int dtype, const void* src, int64_t ld_src, void* dst,
                             int64_t ld_dst, int64_t n, int64_t f, float alpha, hipStream_t s);

// appnp_propagate.hip: what the whole-graph calls share with the step API of appnp_capi.hip.
// set_drop: iteration k's dropout parameters.  vec16: whether every operand allows 16-B vectors.
// remainder_cols: the columns the split layout gives to the remainder pass, 0 for whole rows.
void set_drop(StepArgs& a, float p_drop, uint64_t seed, int k);
bool vec16(const int64_t* lds, int n_ld, const void* const* ptrs, int n_ptr);
int64_t remainder_cols(const appnp_graph* g, int64_t f, int dtype, bool aligned);

// appnp_capi.hip: a tuning override (measurement only, tools/): `name` is read from the
// environment when APPNP_TUNING=1, else dflt.  Each is read once, at its first use; every name
// must be listed in kTuningNames (appnp_capi.hip), which appnp_tuning_overrides reports.
int tuning_env(const char* name, int dflt);

// appnp_capi.hip: the per-launch timer of appnp_kernel_timer_begin / _end.  While it is on
// (on this thread), every launch (or exchange) of the propagation entry points is bracketed by
// two timing events on its stream: ktimer_begin right before it, ktimer_mark right after it,
// tagged with its kind (APPNP_KT_*).  So an interval covers that launch only, never a wait that
// precedes it on the stream.  Off: one thread-local load each.
void ktimer_begin(hipStream_t s);
void ktimer_mark(hipStream_t s, int kind);

inline size_t round_up(size_t x, size_t al) { return (x + al - 1) / al * al; }

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Workgroups of a thread-per-item launch of kBlock threads over n items (at least one).
inline unsigned blocks_for(int64_t n) {
  return n > kBlock ? (unsigned)((n + kBlock - 1) / kBlock) : 1u;
}

// hipError_t -> APPNP_E*, two ways.  build_err is the set-up builders' (graph, blocks, ingest):
// they check their arguments before the first HIP call, so whatever is not an allocation failure
// is the device's.  dev_err is the entry points' (appnp_capi.hip, appnp_propagate.hip,
// appnp_dist.hip), which hand caller-supplied sizes and pointers to the runtime: there
// hipErrorInvalidValue is the caller's mistake, APPNP_EINVAL.
inline int build_err(hipError_t e) {
  if (e == hipSuccess) return APPNP_OK;
  return e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? APPNP_ENOMEM : APPNP_EDEVICE;
}
inline int dev_err(hipError_t e) { return e == hipErrorInvalidValue ? APPNP_EINVAL : build_err(e); }

// Returns build_err(expr) from the enclosing builder when expr fails.  The builder's temporaries
// live in a DeviceScratch and what it keeps lives in the appnp_graph / appnp_csr, which the
// caller releases (graph_free / csr_free), so returning early leaks nothing.
#define APPNP_TRY(expr)                                       \
  do {                                                        \
    const hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return ::appnp::build_err(e_);      \
  } while (0)

// count elements of device memory (one when count <= 0, so an empty input still gets a pointer)
template <class T>
inline hipError_t device_alloc(T** p, int64_t count) {
  *p = nullptr;
  return hipMalloc(reinterpret_cast<void**>(p), (size_t)(count > 0 ? count : 1) * sizeof(T));
}

// The temporary device buffers of one set-up call: freed when the scope ends, on every path.
class DeviceScratch {
 public:
  DeviceScratch() = default;
  DeviceScratch(const DeviceScratch&) = delete;
  DeviceScratch& operator=(const DeviceScratch&) = delete;
  ~DeviceScratch() {
    for (int i = 0; i < n_; ++i) (void)hipFree(ptrs_[i]);
  }
  template <class T>
  hipError_t get(T** p, int64_t count) {
    *p = nullptr;
    if (n_ == kMax) return hipErrorOutOfMemory;  // more buffers than any builder takes
    const hipError_t e = device_alloc(p, count);
    if (e == hipSuccess) ptrs_[n_++] = *p;
    return e;
  }

 private:
  static constexpr int kMax = 16;  // standardize takes 15
  void* ptrs_[kMax];
  int n_ = 0;
};

// One launch (or copy) on `s` between the kernel timer's two events, tagged `kind` (APPNP_KT_*).
// Every launch of the propagation entry points (appnp_propagate.hip, appnp_capi.hip) goes through
// here; `launch` returns its hipError_t.
template <typename Launch>
inline int timed(hipStream_t s, int kind, Launch launch) {
  ktimer_begin(s);
  const int rc = dev_err(launch());
  ktimer_mark(s, kind);
  return rc;
}

inline int timed_step(int dtype, int epi, int V, const StepArgs& a, hipStream_t s,
                      int kind = APPNP_KT_STEP) {
  return timed(s, kind, [&] { return launch_step(dtype, epi, V, a, s); });
}

inline int64_t elem_size(int dtype) { return dtype == APPNP_F32 ? 4 : 2; }

inline bool valid_dtype(int dtype) { return dtype == APPNP_F32 || dtype == APPNP_BF16; }

// Whether an adjoint on `g` needs the transposed CSR built at creation (APPNP_GRAPH_TRANSPOSE):
// always, except for 'sym' on an undirected graph, whose A_hat is its own transpose.
inline bool needs_transpose(const appnp_graph* g) {
  return !(g->mode == APPNP_NORM_SYM && g->symmetric);
}

// The caller's workspace from its 256-B aligned base on.
struct Workspace {
  char* base = nullptr;
  size_t need = 0;  // the bytes taken from the base
  size_t room = 0;  // the bytes the workspace holds from the base, `need` included

  // Take `bytes` from the aligned base; APPNP_EINVAL when they are needed and `ws` is null or too
  // small.  bytes = 0 touches nothing: a caller that needs no workspace may pass none.
  int take(void* ws, size_t ws_bytes, size_t bytes) {
    *this = Workspace{};
    if (bytes == 0) return APPNP_OK;
    if (!ws) return APPNP_EINVAL;
    const uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    const uintptr_t aligned = (p + 255) & ~uintptr_t(255);
    if (ws_bytes < bytes + (aligned - p)) return APPNP_EINVAL;
    base = reinterpret_cast<char*>(aligned);
    need = bytes;
    room = ws_bytes - (aligned - p);
    return APPNP_OK;
  }
  // the buffer at byte `off` of what was taken, null past its end
  void* at(size_t off) const { return off < need ? base + off : nullptr; }
};

// Where a chain of steps stands: what the next step gathers from.
struct Chain {
  const void* src;
  int64_t ld;
  // the next step reads the source and writes `dst` (null: it keeps no rows), the step after
  // that reads `dst`
  void advance(StepArgs& a, void* dst, int64_t ld_dst) {
    a.zin = src;
    a.ld_in = ld;
    a.out = dst;
    a.ld_out = ld_dst;
    src = dst;
    ld = ld_dst;
  }
};

// The step arguments every propagation on the held rows of `g` starts from.
inline StepArgs base_args(const appnp_graph* g, int64_t f, float alpha) {
  StepArgs a{};
  a.row_ptr = g->row_ptr;
  a.col = g->col;
  a.val = g->val;
  a.n_rows = g->row_hi - g->row_lo;
  a.nnz = g->nnz_hat;
  a.nnz_rows = g->nnz_hat;  // a step over part of the rows' entries overrides nnz only
  a.zin_rows = g->n;
  a.row_lo = g->row_lo;
  a.f = (int32_t)f;
  a.scale = 1.0f - alpha;
  a.alpha = alpha;
  a.drop_scale = 1.0f;
  a.heavy = g->heavy;
  a.n_heavy = g->n_heavy;
  a.heavy_thr = kHeavyRow;
  a.hub = g->hub;
  a.n_hub = g->n_hub;
  return a;
}

// A_hat^T for the adjoints of a graph whose A_hat is not symmetric: the transposed CSR built at
// creation (APPNP_GRAPH_TRANSPOSE) and its heavy / hub rows
inline void use_transpose(StepArgs& a, const appnp_graph* g) {
  a.row_ptr = g->t_row_ptr;
  a.col = g->t_col;
  a.val = g->t_val;
  a.heavy = g->t_heavy;
  a.n_heavy = g->t_n_heavy;
  a.hub = g->t_hub;
  a.n_hub = g->t_n_hub;
}

inline int launch_err() { return hipGetLastError() == hipSuccess ? APPNP_OK : APPNP_EDEVICE; }

// One launch of the top-k, push and batch entry points, bracketed for the per-launch timer.
template <typename Launch>
inline int timed_launch(hipStream_t s, int kind, Launch launch) {
  ktimer_begin(s);
  launch();
  const int rc = launch_err();
  ktimer_mark(s, kind);
  return rc;
}

// Leading dimension of the internal ping-pong buffers.  A random row gather costs 128-B line
// requests, not bytes, so rows are padded to start on a line
// (next power of two up to one line, then whole lines) -- but only when that lowers the
// average number of lines a row spans; otherwise (e.g. 400-B fp32 rows: 4 lines either way)
// packed rows avoid a partially written line per row.
inline double avg_lines(int64_t row_bytes, int64_t stride) {
  // rows start at offsets (i * stride) mod 128, periodic
  int64_t g = stride % 128 == 0 ? 128 : stride;
  int64_t a = 128, b = g;
  while (b) { const int64_t t = a % b; a = b; b = t; }
  const int64_t period = 128 / a;
  double sum = 0.0;
  for (int64_t i = 0; i < period; ++i) {
    const int64_t o = (i * stride) % 128;
    sum += (double)((o + row_bytes - 1) / 128 + 1);
  }
  return sum / (double)period;
}

inline int64_t line_ld(int64_t f, int dtype) {
  const int64_t es = dtype == APPNP_F32 ? 4 : 2;
  const int64_t line = 128 / es;
  if (f <= 0) return 1;
  int64_t padded;
  if (f <= line) {
    padded = 1;
    while (padded < f) padded <<= 1;
  } else {
    padded = (f + line - 1) / line * line;
  }
  const int64_t v = es == 4 ? 4 : 8;  // keep 16-B vectors possible for the packed layout
  const int64_t packed = (f + v - 1) / v * v;
  return avg_lines(f * es, padded * es) < avg_lines(f * es, packed * es) ? padded : packed;
}

}  // namespace appnp
