// appnp_capi.hip -- the extern "C" boundary declared in include/ppnp_amd.h, except the whole-graph
// propagation calls and their plans (appnp_propagate.hip).
//
// The graph API, the per-iteration step and shard API (argument validation and one launch each),
// the per-launch timer, the tuning overrides and the build info.  No host synchronisation or
// allocation happens in appnp_step and its kin, so a caller may capture them in a hipGraph.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "../../include/ppnp_amd.h"
#include "appnp_internal.h"

using appnp::StepArgs;

namespace appnp {
namespace {

// appnp_kernel_timer_*: two timing events per launch, recorded on the launch's stream right
// before and right after it
struct KTimer {
  bool on = false;
  int dropped = 0;              // launches past the capacity (not timed)
  std::vector<hipEvent_t> ev;   // ev[2 i]: before launch i; ev[2 i + 1]: after it
  std::vector<int> kind;
  int n = 0;                    // launches recorded
  bool open = false;            // ev[2 n] recorded, its launch's end not yet
  bool over = false;            // the launch begun now is past the capacity
  hipStream_t open_s = nullptr;

  void release() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
    kind.clear();
    n = dropped = 0;
    on = open = over = false;
    open_s = nullptr;
  }
};
thread_local KTimer g_ktimer;

}  // namespace

void ktimer_begin(hipStream_t s) {
  KTimer& t = g_ktimer;
  if (!t.on) return;
  t.open = false;
  t.over = 2 * t.n + 1 >= (int)t.ev.size();
  if (!t.over && hipEventRecord(t.ev[2 * t.n], s) == hipSuccess) {
    t.open = true;
    t.open_s = s;
  }
}

void ktimer_mark(hipStream_t s, int kind) {
  KTimer& t = g_ktimer;
  if (!t.on) return;
  if (t.over) {
    ++t.dropped;
    t.over = false;
    return;
  }
  if (!t.open || t.open_s != s) return;  // no begin on this stream: not a timed launch
  t.open = false;
  if (hipEventRecord(t.ev[2 * t.n + 1], s) != hipSuccess) {
    ++t.dropped;
    return;
  }
  t.kind[t.n] = kind;
  ++t.n;
}

// Every tuning override the library reads (tuning_env).  They change which kernel variant runs
// or how it is shaped, never results beyond fp32 summation order, and exist for the sweeps of
// tools/; a product run leaves APPNP_TUNING unset and gets the measured defaults.
const char* const kTuningNames[] = {
    "APPNP_SPLIT",       "APPNP_VEC",         "APPNP_WIDE",         "APPNP_UW",
    "APPNP_UN",          "APPNP_NT",          "APPNP_MAX_BLOCKS",   "APPNP_REM_SYNC_W4",
    "APPNP_REM_SYNC_W8", "APPNP_REM_SYNC_W16", "APPNP_SB_ROWS",     "APPNP_REM_VF"};

bool tuning_on() {
  static const bool on = [] {
    const char* v = getenv("APPNP_TUNING");
    return v && v[0] == '1' && v[1] == '\0';
  }();
  return on;
}

int tuning_env(const char* name, int dflt) {
  if (!tuning_on()) return dflt;
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

}  // namespace appnp

namespace {

using namespace appnp;

// What every step entry point checks first
int check_step(const appnp_graph* g, int64_t f, int dtype, float alpha, float p_drop) {
  if (!g) return APPNP_EINVAL;
  if (f < 0 || f > INT32_MAX || !valid_dtype(dtype)) return APPNP_EINVAL;
  if (!(alpha >= 0.0f && alpha <= 1.0f)) return APPNP_EINVAL;
  if (!(p_drop >= 0.0f && p_drop < 1.0f)) return APPNP_EINVAL;
  return APPNP_OK;
}

// The heavy / hub lists describe the whole held rows: a step over part of their entries (the
// LOCAL / REMOTE half, a shard range) runs without them.
void drop_row_lists(StepArgs& a) {
  a.heavy = nullptr;
  a.n_heavy = 0;
  a.hub = nullptr;
  a.n_hub = 0;
}

}  // namespace

extern "C" {

int appnp_abi_version(void) { return PPNP_AMD_ABI_VERSION; }

#ifndef APPNP_SRC_DIGEST
#define APPNP_SRC_DIGEST "unknown"
#endif
#define APPNP_STR2(x) #x
#define APPNP_STR(x) APPNP_STR2(x)

#ifndef APPNP_ARCH
#define APPNP_ARCH "unknown"
#endif

const char* appnp_build_info(void) {
  return "src=" APPNP_SRC_DIGEST ";abi=" APPNP_STR(PPNP_AMD_ABI_VERSION) ";arch=" APPNP_ARCH
#ifdef APPNP_TESTING
      ";testing=1"
#endif
      ";compiler=" __VERSION__ ";built=" __DATE__ " " __TIME__;
}

const char* appnp_strerror(int code) {
  switch (code) {
    case APPNP_OK: return "ok";
    case APPNP_EDEVICE: return "HIP device error";
    case APPNP_ENOMEM: return "out of device memory";
    case APPNP_EINVAL: return "invalid argument";
    case APPNP_ERANGE: return "size exceeds int32 CSR index range";
    case APPNP_ENOTSUP: return "not supported";
    default: return "unknown error";
  }
}

int appnp_graph_create_rows(const int32_t* indptr, const int32_t* indices, const float* vals,
                            int64_t n, int64_t nnz, int mode, int64_t row_lo, int64_t row_hi,
                            int split_local, void* stream, appnp_graph** out) {
  if (!out) return APPNP_EINVAL;
  *out = nullptr;
  if (n < 0 || nnz < 0 || n > INT32_MAX || nnz > INT32_MAX) return n > INT32_MAX || nnz > INT32_MAX ? APPNP_ERANGE : APPNP_EINVAL;
  const bool want_t = (mode & APPNP_GRAPH_TRANSPOSE) != 0;
  // remainder width of the source-blocked copy: 4 columns, or 8 / 16 (APPNP_GRAPH_SB_W8 / _W16)
  const int sb_lpe = (mode & APPNP_GRAPH_SB_W16) ? 4 : (mode & APPNP_GRAPH_SB_W8) ? 2 : 1;
  const bool want_sb = (mode & (APPNP_GRAPH_SOURCE_BLOCKS | APPNP_GRAPH_SB_W8 |
                                APPNP_GRAPH_SB_W16)) != 0;
  mode &= ~(APPNP_GRAPH_TRANSPOSE | APPNP_GRAPH_SOURCE_BLOCKS | APPNP_GRAPH_SB_W8 |
            APPNP_GRAPH_SB_W16);
  if (mode != APPNP_NORM_SYM && mode != APPNP_NORM_RW) return APPNP_EINVAL;
  if (row_lo < 0 || row_hi < row_lo || row_hi > n) return APPNP_EINVAL;
  if (want_t && (row_lo != 0 || row_hi != n)) return APPNP_EINVAL;
  if (n > 0 && !indptr) return APPNP_EINVAL;
  if (nnz > 0 && !indices) return APPNP_EINVAL;
  appnp_graph* g = new (std::nothrow) appnp_graph();
  if (!g) return APPNP_ENOMEM;
  int rc = appnp::graph_build(indptr, indices, vals, n, nnz, mode, row_lo, row_hi,
                              split_local, as_stream(stream), g);
  // A_hat^T for the adjoints, where they need it
  if (rc == APPNP_OK && want_t && needs_transpose(g))
    rc = appnp::graph_build_transpose(g, as_stream(stream));
  // source-blocked copy for the remainder pass (appnp_propagate on a full graph,
  // appnp_step_split on the held rows of a row-partitioned one).  Best-effort: a graph too
  // large for the copy (block or segment count, device memory) keeps whole-row gathers --
  // appnp_graph_source_blocks reports whether it was built.
  if (rc == APPNP_OK && want_sb) {
    const int sb =
        appnp::graph_build_source_blocks(g, sb_lpe, indptr, indices, nnz, as_stream(stream));
    if (sb != APPNP_OK && sb != APPNP_ENOTSUP && sb != APPNP_ERANGE && sb != APPNP_ENOMEM)
      rc = sb;
  }
  if (rc != APPNP_OK) {
    appnp::graph_free(g);
    delete g;
    return rc;
  }
  *out = g;
  return APPNP_OK;
}

int appnp_graph_create(const int32_t* indptr, const int32_t* indices, const float* vals,
                       int64_t n, int64_t nnz, int mode, void* stream, appnp_graph** out) {
  return appnp_graph_create_rows(indptr, indices, vals, n, nnz, mode, 0, n, 0, stream, out);
}

void appnp_graph_destroy(appnp_graph* g) {
  if (!g) return;
  appnp::graph_free(g);
  delete g;
}

int appnp_graph_info(const appnp_graph* g, int64_t* n, int64_t* row_lo, int64_t* row_hi,
                     int64_t* nnz_hat, int* mode, int* symmetric) {
  if (!g) return APPNP_EINVAL;
  if (n) *n = g->n;
  if (row_lo) *row_lo = g->row_lo;
  if (row_hi) *row_hi = g->row_hi;
  if (nnz_hat) *nnz_hat = g->nnz_hat;
  if (mode) *mode = g->mode;
  if (symmetric) *symmetric = g->symmetric;
  return APPNP_OK;
}

int appnp_graph_csr(const appnp_graph* g, const int32_t** row_ptr, const int32_t** col,
                    const float** val) {
  if (!g) return APPNP_EINVAL;
  if (row_ptr) *row_ptr = g->row_ptr;
  if (col) *col = g->col;
  if (val) *val = g->val;
  return APPNP_OK;
}

int appnp_graph_copy_csr(const appnp_graph* g, int32_t* row_ptr, int32_t* col, float* val,
                         double* dinv, void* stream) {
  if (!g) return APPNP_EINVAL;
  const hipStream_t s = as_stream(stream);
  const int64_t rows = g->row_hi - g->row_lo;
  hipError_t e = hipSuccess;
  if (row_ptr && e == hipSuccess)
    e = hipMemcpyAsync(row_ptr, g->row_ptr, (rows + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
  if (col && g->nnz_hat && e == hipSuccess)
    e = hipMemcpyAsync(col, g->col, g->nnz_hat * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
  if (val && g->nnz_hat && e == hipSuccess)
    e = hipMemcpyAsync(val, g->val, g->nnz_hat * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (dinv && g->n && e == hipSuccess)
    e = hipMemcpyAsync(dinv, g->dinv, g->n * sizeof(double), hipMemcpyDeviceToDevice, s);
  return dev_err(e);
}

int appnp_graph_dinv(const appnp_graph* g, const double** dinv) {
  if (!g || !dinv) return APPNP_EINVAL;
  *dinv = g->dinv;
  return APPNP_OK;
}

int appnp_graph_source_blocks(const appnp_graph* g, int64_t* bytes) {
  if (!g || !bytes) return APPNP_EINVAL;
  *bytes = 0;
  if (g->rb_off)
    *bytes = g->rb_total * (g->rb_val ? 8 : 4) + g->rb_total / 16 * g->rb_lpe +
             ((int64_t)g->rb_passes * g->rb_nb * g->rb_slots + 1) * (int64_t)sizeof(int32_t) +
             (g->rb_dl ? g->n * 4 : 0) + (g->rb_dr ? g->n * 4 : 0);
  return APPNP_OK;
}

int appnp_graph_source_block_layout(const appnp_graph* g, int* width, int64_t* entries,
                                    int* value_free, int* row_passes, int64_t* launches) {
  if (!g) return APPNP_EINVAL;
  const bool built = g->rb_off != nullptr;
  if (width) *width = built ? 4 * g->rb_lpe : 0;
  if (entries) *entries = built ? g->rb_total : 0;
  if (value_free) *value_free = built && g->rb_val == nullptr ? 1 : 0;
  if (row_passes) *row_passes = built ? g->rb_passes : 0;
  if (launches) *launches = g->rem_launches.load(std::memory_order_relaxed);
  return APPNP_OK;
}

int appnp_spmm(const int32_t* indptr, const int32_t* indices, const float* vals, int64_t rows,
               int64_t cols, const float* B, int64_t ld_b, float* Cm, int64_t ld_c, int64_t f,
               float p_drop, uint64_t seed, int transposed_key, void* stream) {
  if (rows < 0 || cols < 0 || f < 0 || f > INT32_MAX) return APPNP_EINVAL;
  if (!(p_drop >= 0.0f && p_drop < 1.0f)) return APPNP_EINVAL;
  if (rows == 0 || f == 0) return APPNP_OK;
  if (!indptr || !Cm || ld_c < f || (cols > 0 && (!B || ld_b < f))) return APPNP_EINVAL;
  StepArgs a{};
  a.row_ptr = indptr;
  a.col = indices;
  a.val = vals;
  a.zin = B;
  a.ld_in = ld_b;
  a.out = Cm;
  a.ld_out = ld_c;
  a.n_rows = rows;
  a.nnz = -1;  // not known on the host without a device read
  a.zin_rows = cols;
  a.row_lo = 0;
  a.f = (int32_t)f;
  a.scale = 1.0f;
  a.alpha = 0.0f;
  a.tkey = transposed_key ? 1 : 0;
  set_drop(a, p_drop, seed, 0);
  const int64_t lds[2] = {ld_b, ld_c};
  const void* ptrs[2] = {B, Cm};
  const int V = appnp::pick_vec(APPNP_F32, f, lds, 2, ptrs, 2);
  return dev_err(appnp::launch_step(APPNP_F32, appnp::EPI_PARTIAL, V, a, as_stream(stream)));
}

// ---- per-iteration steps ------------------------------------------------------------------
//
// appnp_step, appnp_step_split, appnp_step_shards and appnp_step_split_shards are one operation:
// the SpMM step over some of the held rows' entries, in one of four roles -- produce a partial
// (SHARDS_FIRST, PART_LOCAL), add to it (SHARDS_ACC), finish the row from it (SHARDS_LAST,
// PART_REMOTE), or do the whole row (SHARDS_ONLY, PART_ALL).  Each entry point keeps its own
// early checks and operand names; which entries it multiplies, and in which role, is a StepPart.

namespace {

struct StepPart {
  const int32_t* row_ptr;
  const int32_t* row_end;  // null: row i's entries end at row_ptr[i + 1]
  const int32_t* col;
  const float* val;
  int64_t nnz;         // the entries (of a shard range: its uniform share): picks the row shape
  bool whole;          // every entry of the held rows, so their heavy / hub lists apply
  int epi;
  int kind;            // APPNP_KT_* of the step's launch
  bool to_partial;     // the product goes to the fp32 partial: no H yet, no output row
  bool reads_partial;  // the product continues from the partial
  bool finishes() const { return !to_partial; }  // the output row: + alpha H
};

// The entries of `part` (appnp_part): the held rows' CSR, or its local / remote half.
int part_of(const appnp_graph* g, int part, int dtype, StepPart* p) {
  *p = StepPart{g->row_ptr, nullptr, g->col, g->val, g->nnz_hat, true,
                appnp::EPI_FWD, APPNP_KT_STEP, false, false};
  if (part == APPNP_PART_ALL) return APPNP_OK;
  if (!g->split) return APPNP_EINVAL;
  if (dtype != APPNP_F32) return APPNP_ENOTSUP;
  if (part == APPNP_PART_LOCAL)
    *p = StepPart{g->lrow_ptr, nullptr, g->lcol, g->lval, g->nnz_local, false,
                  appnp::EPI_PARTIAL, APPNP_KT_LOCAL, true, false};
  else if (part == APPNP_PART_REMOTE)
    *p = StepPart{g->rrow_ptr, nullptr, g->rcol, g->rval, g->nnz_remote, false,
                  appnp::EPI_FINISH, APPNP_KT_REMOTE, false, true};
  else
    return APPNP_EINVAL;
  return APPNP_OK;
}

// The held rows' entries with a column in shards [s_lo, s_hi), in the role of `mode`
// (appnp_shard_mode): FIRST partial = y, ACC partial += y, LAST out = y + partial + alpha H,
// ONLY out = y + alpha H.
int shards_of(const appnp_graph* g, int s_lo, int s_hi, int mode, StepPart* p) {
  if (!g->sh_off) return APPNP_EINVAL;  // appnp_graph_shard_offsets first
  if (s_lo < 0 || s_hi > g->sh_n || s_lo >= s_hi) return APPNP_EINVAL;
  const int64_t rows = g->row_hi - g->row_lo;
  // the kernel shape follows the average row length: the range's share of the entries
  *p = StepPart{g->sh_off + (int64_t)s_lo * rows, g->sh_off + (int64_t)s_hi * rows, g->col,
                g->val, g->nnz_hat * (int64_t)(s_hi - s_lo) / g->sh_n, false,
                appnp::EPI_FWD, APPNP_KT_REMOTE, false, false};
  switch (mode) {
    case APPNP_SHARDS_FIRST:
      p->epi = appnp::EPI_PARTIAL;
      p->kind = APPNP_KT_LOCAL;
      p->to_partial = true;
      return APPNP_OK;
    case APPNP_SHARDS_ACC:
      p->epi = appnp::EPI_ACCUM;
      p->to_partial = p->reads_partial = true;
      return APPNP_OK;
    case APPNP_SHARDS_LAST:
      p->epi = appnp::EPI_FINISH;
      p->reads_partial = true;
      return APPNP_OK;
    case APPNP_SHARDS_ONLY: return APPNP_OK;
    default: return APPNP_EINVAL;
  }
}

// base_args over the entries of `p`, with iteration k's dropout
StepArgs part_args(const appnp_graph* g, const StepPart& p, int64_t f, int k, float alpha,
                   float p_drop, uint64_t seed) {
  StepArgs a = base_args(g, f, alpha);
  a.row_ptr = p.row_ptr;
  a.row_end = p.row_end;
  a.col = p.col;
  a.val = p.val;
  a.nnz = p.nnz;
  if (!p.whole) drop_row_lists(a);
  set_drop(a, p_drop, seed, k);
  return a;
}

// What a whole-row step reads beside Zin: H where it finishes the row, the partial where it
// continues from one
int check_reads(const StepPart& p, const void* H, int64_t ld_h, const float* partial,
                int64_t ld_partial, int64_t f) {
  if (p.finishes() && (!H || ld_h < f)) return APPNP_EINVAL;
  if (p.reads_partial && (!partial || ld_partial < f)) return APPNP_EINVAL;
  return APPNP_OK;
}

// The whole-row step of `p` at vector width V, into `out`: the caller's output rows, or its
// partial where p.to_partial.
int step_rows(const appnp_graph* g, const StepPart& p, int dtype, int V, const void* Zin,
              int64_t ld_in, const void* H, int64_t ld_h, void* out, int64_t ld_out,
              const float* partial, int64_t ld_partial, int64_t f, int k, float alpha,
              float p_drop, uint64_t seed, hipStream_t s) {
  StepArgs a = part_args(g, p, f, k, alpha, p_drop, seed);
  a.zin = Zin;
  a.ld_in = ld_in;
  a.out = out;
  a.ld_out = ld_out;
  if (p.finishes()) {
    a.h = H;
    a.ld_h = ld_h;
    if (p.reads_partial) {
      a.aux = const_cast<float*>(partial);
      a.ld_aux = ld_partial;
    }
  }
  return timed_step(dtype, p.epi, V, a, s, p.kind);
}

// remainder columns of a held-rows split step (appnp_step_split / appnp_split_copy); 0: none
int64_t rows_split(const appnp_graph* g, int64_t f) {
  return g ? remainder_cols(g, f, APPNP_F32, true) : 0;
}

// The step of `p` in the split layout of the held rows (remainder columns r): the main launch
// on the fs = f - r main columns, then, where p finishes the row, the remainder pass.
int step_split_rows(const appnp_graph* g, const StepPart& p, int64_t r, const float* zin_main,
                    const float* zin_rem, const float* H, int64_t ld_h, float* zout_main,
                    float* zout_rem, float* Z, int64_t ld_z, float* partial, int64_t ld_partial,
                    int64_t f, int k, float alpha, float p_drop, uint64_t seed, hipStream_t s) {
  const int64_t fs = f - r, rw = 4 * (int64_t)g->rb_lpe;
  const bool to_z = Z != nullptr;
  const bool uses_partial = p.to_partial || p.reads_partial;
  // inputs: every row of both parts (the remainder only where the pass runs)
  if (fs > 0 && !zin_main) return APPNP_EINVAL;
  if (p.finishes() && (!zin_rem || !H || ld_h < f)) return APPNP_EINVAL;
  if (p.finishes() && !to_z && (!zout_rem || (fs > 0 && !zout_main))) return APPNP_EINVAL;
  if (to_z && ld_z < f) return APPNP_EINVAL;
  if (uses_partial && (!partial || ld_partial < fs)) return APPNP_EINVAL;
  const int64_t lds[3] = {p.finishes() ? ld_h : 4, to_z ? ld_z : 4, uses_partial ? ld_partial : 4};
  const void* ptrs[7] = {zin_main, zin_rem, H, zout_main, zout_rem, Z, partial};
  if (!vec16(lds, 3, ptrs, 7)) return APPNP_EINVAL;
  if (fs > 0) {
    StepArgs am = part_args(g, p, fs, k, alpha, p_drop, seed);
    am.zin = zin_main;
    am.ld_in = fs;
    if (p.to_partial) {
      am.out = partial;
      am.ld_out = ld_partial;
    } else {
      am.out = to_z ? Z : zout_main + g->row_lo * fs;
      am.ld_out = to_z ? ld_z : fs;
      am.h = H;
      am.ld_h = ld_h;
      if (p.reads_partial) {
        am.aux = partial;
        am.ld_aux = ld_partial;
      }
    }
    const int rc = timed_step(APPNP_F32, p.epi, 4, am, s, p.kind);
    if (rc) return rc;
  }
  if (!p.finishes()) return APPNP_OK;  // the pass needs every row of zin_rem
  // the remainder pass over every source block: into the next remainder buffer at the held
  // rows (a unit graph stores dr o y there), or into Z's last r columns
  StepArgs a = base_args(g, f, alpha);
  set_drop(a, p_drop, seed, k);
  const int nv = (g->rb_lpe == 1 && !to_z) ? 4 : (int)r;
  g->rem_launches.fetch_add(1, std::memory_order_relaxed);
  return timed(s, APPNP_KT_REM, [&] {
    return appnp::launch_remainder(g, a, appnp::EPI_FWD, zin_rem, H + fs, ld_h,
                                   to_z ? Z + fs : zout_rem + g->row_lo * rw, to_z ? ld_z : rw,
                                   nv, !to_z, s);
  });
}

}  // namespace

int appnp_step(const appnp_graph* g, int part, const void* Zin, int64_t ld_in, const void* H,
               int64_t ld_h, void* Zout, int64_t ld_out, const float* partial,
               int64_t ld_partial, int64_t f, int dtype, int k, float alpha, float p_drop,
               uint64_t seed, void* stream) {
  int rc = check_step(g, f, dtype, alpha, p_drop);
  if (rc) return rc;
  if (k < 0) return APPNP_EINVAL;
  if (g->row_hi == g->row_lo || f == 0) return APPNP_OK;
  if (!Zin || !Zout || ld_in < f || ld_out < f) return APPNP_EINVAL;
  StepPart p;
  if ((rc = part_of(g, part, dtype, &p))) return rc;
  if ((rc = check_reads(p, H, ld_h, partial, ld_partial, f))) return rc;
  // every pointer counts whatever the part reads, the leading dimensions only of what it reads;
  // PART_LOCAL's partial is Zout
  const int64_t lds[4] = {ld_in, ld_out, ld_h, ld_partial};
  const void* ptrs[4] = {Zin, Zout, H, partial};
  const int n_ld = p.reads_partial ? 4 : p.finishes() ? 3 : 2;
  const int V = appnp::pick_vec(dtype, f, lds, n_ld, ptrs, 4);
  return step_rows(g, p, dtype, V, Zin, ld_in, H, ld_h, Zout, ld_out, partial, ld_partial, f, k,
                   alpha, p_drop, seed, as_stream(stream));
}

// ---- the split layout on the held rows of a row-partitioned graph -------------------------

int appnp_split_layout(const appnp_graph* g, int64_t f, int64_t* fs, int64_t* rem_width) {
  if (!g || f < 0) return APPNP_EINVAL;
  const int64_t r = rows_split(g, f);
  if (fs) *fs = r ? f - r : 0;
  if (rem_width) *rem_width = r ? 4 * (int64_t)g->rb_lpe : 0;
  return r ? APPNP_OK : APPNP_ENOTSUP;
}

int appnp_split_copy(const appnp_graph* g, const float* H, int64_t ld_h, int64_t f, float* main,
                     float* rem, void* stream) {
  if (!g || f <= 0) return APPNP_EINVAL;
  const int64_t r = rows_split(g, f);
  if (!r) return APPNP_ENOTSUP;
  const int64_t rows = g->row_hi - g->row_lo, fs = f - r, rw = 4 * (int64_t)g->rb_lpe;
  if (rows == 0) return APPNP_OK;
  const int64_t lds[1] = {ld_h};
  const void* ptrs[3] = {H, main, rem};
  if (!H || !rem || (fs > 0 && !main) || ld_h < f || !vec16(lds, 1, ptrs, 3)) return APPNP_EINVAL;
  const float* sc = appnp::remainder_scale(g);
  const hipStream_t s = as_stream(stream);
  return timed(s, APPNP_KT_COPY, [&] {
    return appnp::launch_split_copy(H, ld_h, rows, f, fs, rw,
                                    main ? main + g->row_lo * fs : nullptr, rem + g->row_lo * rw,
                                    sc ? sc + g->row_lo : nullptr, s);
  });
}

int appnp_step_split(const appnp_graph* g, int part, const float* zin_main, const float* zin_rem,
                     const float* H, int64_t ld_h, float* zout_main, float* zout_rem, float* Z,
                     int64_t ld_z, float* partial, int64_t ld_partial, int64_t f, int k,
                     float alpha, float p_drop, uint64_t seed, void* stream) {
  int rc = check_step(g, f, APPNP_F32, alpha, p_drop);
  if (rc) return rc;
  if (k < 0 || part < APPNP_PART_ALL || part > APPNP_PART_REMOTE) return APPNP_EINVAL;
  const int64_t r = rows_split(g, f);
  if (!r) return APPNP_ENOTSUP;
  if (g->row_hi == g->row_lo || f == 0) return APPNP_OK;
  StepPart p;
  if ((rc = part_of(g, part, APPNP_F32, &p))) return rc;
  if (part != APPNP_PART_ALL && r == f) return APPNP_EINVAL;  // no main columns to halve
  return step_split_rows(g, p, r, zin_main, zin_rem, H, ld_h, zout_main, zout_rem, Z, ld_z,
                         partial, ld_partial, f, k, alpha, p_drop, seed, as_stream(stream));
}

// ---- pipelined row steps: the held rows' entries of a range of source shards -------------

int appnp_graph_shard_offsets(appnp_graph* g, int nshards, int64_t shard_rows, void* stream) {
  if (!g) return APPNP_EINVAL;
  return appnp::graph_build_shard_offsets(g, nshards, shard_rows, as_stream(stream));
}

int appnp_step_shards(const appnp_graph* g, int s_lo, int s_hi, int mode, const float* Zin,
                      int64_t ld_in, const float* H, int64_t ld_h, float* Zout, int64_t ld_out,
                      float* partial, int64_t ld_partial, int64_t f, int k, float alpha,
                      float p_drop, uint64_t seed, void* stream) {
  int rc = check_step(g, f, APPNP_F32, alpha, p_drop);
  if (rc) return rc;
  if (k < 0) return APPNP_EINVAL;
  StepPart p;
  if ((rc = shards_of(g, s_lo, s_hi, mode, &p))) return rc;
  if (g->row_hi == g->row_lo || f == 0) return APPNP_OK;
  // FIRST / ACC write the partial, LAST / ONLY the output rows
  void* const out = p.to_partial ? static_cast<void*>(partial) : static_cast<void*>(Zout);
  const int64_t ld = p.to_partial ? ld_partial : ld_out;
  if (!Zin || ld_in < f || !out || ld < f) return APPNP_EINVAL;
  if ((rc = check_reads(p, H, ld_h, partial, ld_partial, f))) return rc;
  const int64_t lds[4] = {ld_in, ld, p.finishes() ? ld_h : ld_in,
                          p.reads_partial ? ld_partial : ld_in};
  const void* ptrs[4] = {Zin, out, p.finishes() ? H : nullptr,
                         p.reads_partial ? partial : nullptr};
  const int V = appnp::pick_vec(APPNP_F32, f, lds, 4, ptrs, 4);
  return step_rows(g, p, APPNP_F32, V, Zin, ld_in, H, ld_h, out, ld, partial, ld_partial, f, k,
                   alpha, p_drop, seed, as_stream(stream));
}

int appnp_step_split_shards(const appnp_graph* g, int s_lo, int s_hi, int mode,
                            const float* zin_main, const float* zin_rem, const float* H,
                            int64_t ld_h, float* zout_main, float* zout_rem, float* Z,
                            int64_t ld_z, float* partial, int64_t ld_partial, int64_t f, int k,
                            float alpha, float p_drop, uint64_t seed, void* stream) {
  int rc = check_step(g, f, APPNP_F32, alpha, p_drop);
  if (rc) return rc;
  if (k < 0) return APPNP_EINVAL;
  const int64_t r = rows_split(g, f);
  if (!r) return APPNP_ENOTSUP;
  StepPart p;
  if ((rc = shards_of(g, s_lo, s_hi, mode, &p))) return rc;
  if (g->row_hi == g->row_lo || f == 0) return APPNP_OK;
  if (r == f && mode != APPNP_SHARDS_ONLY) return APPNP_EINVAL;  // nothing to pipeline
  return step_split_rows(g, p, r, zin_main, zin_rem, H, ld_h, zout_main, zout_rem, Z, ld_z,
                         partial, ld_partial, f, k, alpha, p_drop, seed, as_stream(stream));
}

// ---- the per-launch timer (measurement aid; include/ppnp_amd.h) ----------------------------

int appnp_kernel_timer_begin(int max_launches, void* stream) {
  appnp::KTimer& t = appnp::g_ktimer;
  if (max_launches < 1 || max_launches > (1 << 20)) return APPNP_EINVAL;
  t.release();
  t.ev.assign(2 * (size_t)max_launches, nullptr);
  t.kind.assign((size_t)max_launches, 0);
  for (hipEvent_t& e : t.ev) {
    if (hipEventCreate(&e) != hipSuccess) {
      e = nullptr;
      t.release();
      return APPNP_EDEVICE;
    }
  }
  t.on = true;
  (void)stream;  // every launch is bracketed by events on its own stream (ktimer_begin / _mark)
  return APPNP_OK;
}

int appnp_kernel_timer_end(float* ms, int* kinds, int max, int* n_out) {
  appnp::KTimer& t = appnp::g_ktimer;
  if (!t.on) return APPNP_EINVAL;
  t.on = false;
  int rc = APPNP_OK;
  for (int i = 0; i < 2 * t.n && rc == APPNP_OK; ++i)
    rc = dev_err(hipEventSynchronize(t.ev[i]));
  for (int i = 0; i < t.n && i < max && rc == APPNP_OK; ++i) {
    float e = NAN;
    if (hipEventElapsedTime(&e, t.ev[2 * i], t.ev[2 * i + 1]) != hipSuccess) e = NAN;
    if (ms) ms[i] = e;
    if (kinds) kinds[i] = t.kind[i];
  }
  if (n_out) *n_out = t.n;
  if (rc == APPNP_OK && t.dropped) rc = APPNP_ERANGE;
  t.release();
  return rc;
}

// ---- tuning overrides (include/ppnp_amd.h) ------------------------------------------------

const char* appnp_tuning_overrides(void) {
  static const std::string s = [] {
    std::string out;
    if (!appnp::tuning_on()) return out;
    for (const char* name : appnp::kTuningNames) {
      const char* v = getenv(name);
      if (!v || !*v) continue;
      if (!out.empty()) out += ';';
      out += name;
      out += '=';
      out += v;
    }
    return out;
  }();
  return s.c_str();
}

const char* appnp_tuning_names(void) {
  static const std::string s = [] {
    std::string out;
    for (const char* name : appnp::kTuningNames) {
      if (!out.empty()) out += ';';
      out += name;
    }
    return out;
  }();
  return s.c_str();
}
}  // extern "C"
