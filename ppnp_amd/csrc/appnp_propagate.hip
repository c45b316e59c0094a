// appnp_propagate.hip -- the whole-graph propagation calls of include/ppnp_amd.h, side by side:
//
//   appnp_propagate / _bwd   Z = APPNP_K(H), the K-step series, and its adjoint
//   appnp_solve / _bwd       Z = Pi H by Chebyshev semi-iteration, and the same solve on A_hat^T
//   appnp_poly / _bwd        Z = sum_k gamma_k A_hat^k H, gamma in device memory, and its adjoint
//
// and the captured plans that replay the first two as hipGraphs.  The unit holds no kernel: one
// argument check (check_chain), the caller's workspace (Workspace) and each family's launch
// sequence, a chain of steps advanced by Chain.  No host synchronisation or allocation happens
// in any of the six calls, so a caller may capture them in a hipGraph.
#include <algorithm>
#include <climits>
#include <cmath>
#include <new>

#include "../../include/ppnp_amd.h"
#include "appnp_internal.h"

namespace appnp {

// Per-iteration dropout parameters (identical to oracle/ppnp_oracle.py edge_keep_mask).
void set_drop(StepArgs& a, float p_drop, uint64_t seed, int k) {
  if (p_drop > 0.0f) {
    a.mkey = splitmix64(seed + (uint64_t)(k + 1) * 0x9E3779B97F4A7C15ull);
    double thr = (double)p_drop * (double)(1u << 24);
    a.drop_thr = (uint32_t)thr;
    a.drop_on = 1;  // even when the 24-bit threshold rounds to 0, kept edges are rescaled
    a.drop_scale = 1.0f / (1.0f - p_drop);
  } else {
    a.mkey = 0;
    a.drop_thr = 0u;
    a.drop_on = 0;
    a.drop_scale = 1.0f;
  }
}

// Whether every operand allows 16-B vectors: leading dimensions multiples of 4 floats and
// 16-B aligned base pointers (null pointers ignored).  The split path reads and writes H / Z
// (dZ / dH) in 16-B pieces: the split copy, the main kernel at V = 4 and the remainder epilogue.
bool vec16(const int64_t* lds, int n_ld, const void* const* ptrs, int n_ptr) {
  for (int i = 0; i < n_ld; ++i)
    if (lds[i] % 4) return false;
  for (int i = 0; i < n_ptr; ++i)
    if (ptrs[i] && (reinterpret_cast<uintptr_t>(ptrs[i]) % 16)) return false;
  return true;
}

constexpr double kSplitMaxNear = 0.5;  // split rows only below this gather locality

// Split rows (appnp_blocks.hip): the remainder columns r of fp32 rows of F = 32q + r features run
// as a separate chain of persistent L2-resident passes over the source-blocked A_hat, and the
// main part f - r (a multiple of 32, possibly 0) gathers whole lines from the split layout
// [n, 32q].  1-4 columns on a graph built with APPNP_GRAPH_SOURCE_BLOCKS, up to 8 with
// APPNP_GRAPH_SB_W8; narrow rows (f <= 4 rb_lpe: 4 / 8 / 16 with _W16) run wholly in the pass.
// Returns 0 (rows gathered whole) when the path does not apply: no blocked copy, bf16,
// latency-regime graph, F outside [1, 256], operands that do not allow 16-B vectors
// (``aligned``), or a graph with gather locality.  APPNP_SPLIT=0 disables it (measurement).
int64_t remainder_cols(const appnp_graph* g, int64_t f, int dtype, bool aligned) {
  static const int enabled = tuning_env("APPNP_SPLIT", 1);
  if (!enabled || !g->rb_off || dtype != APPNP_F32 || !aligned) return 0;
  if (g->n <= (1 << 16) || f < 1 || f > 256) return 0;
  // graphs with gather locality keep whole rows: their last line is mostly an L2 hit, cheaper
  // than the remainder pass (products-local, ~90 % near entries: 4.0 ms whole rows, 3.7 ms for
  // the 3-line main part alone, 8.5 ms split).  Uniform products-synth: 1.3 % near.
  if (g->near_frac > kSplitMaxNear && enabled != 2) return 0;  // APPNP_SPLIT=2: regardless
  const int64_t w = 4 * (int64_t)g->rb_lpe;
  const int64_t r = f > 32 ? f % 32 : f;
  if (f <= 32 && f > w) return 0;  // one line per row already, or too wide for the pass
  // beside a main part, a remainder of 9-16 columns costs as much as its extra line
  // (products-synth F = 47: 4.53 ms split against 4.41 ms whole rows; F = 40 = 32 + 8: 3.68
  // against 4.44 ms; profiles/r2_wide_remainder.txt)
  if (f > 32 && r > 8) return 0;
  // and beside a main part, the 4-lane pass of a W16 copy (4 row passes) costs more than the
  // extra line even for r <= 4 (products-synth F = 100: 9.44 ms split on W16 against 9.20 whole
  // rows and 7.77 on W4; F = 36: 4.50 against 4.42; profiles/r3_wide_copy_f100.txt).
  // A W8 copy still wins there (F = 100: 8.21 ms), so only W16 keeps whole rows
  if (f > 32 && g->rb_lpe == 4) return 0;
  return (r >= 1 && r <= w) ? r : 0;
}

}  // namespace appnp

namespace {

using namespace appnp;

constexpr int kSolveMaxIters = 1 << 20;
constexpr int kPolyMaxK = APPNP_POLY_MAX_K;

// What an entry point allows beyond the rules all six share (check_chain).
struct ChainRules {
  int min_steps, max_steps;  // of K / iters
  bool alpha_zero;           // alpha = 0 is valid (the solver needs alpha > 0)
  bool f32_only;
  bool undirected_only;
  bool transposed;           // runs on A_hat^T
  bool has_extra = false;    // `extra` is a further pointer that must not be null (poly's coef)
  const void* extra = nullptr;
};

// The argument checks of the six propagation calls, before any device call: the same steps in
// the same order, EINVAL for what is wrong before ENOTSUP for what is not offered.  *run = 0:
// valid and nothing to do (an empty graph or F = 0), whatever the pointers are.  A call without
// dropout passes p_drop = 0, one without alpha passes 0 and allows it.
int check_chain(const appnp_graph* g, const void* in, int64_t ld_in, const void* out,
                int64_t ld_out, int64_t f, int dtype, int steps, float alpha, float p_drop,
                ChainRules r, int* run) {
  *run = 0;
  if (!g) return APPNP_EINVAL;
  if (f < 0 || f > INT32_MAX || steps < r.min_steps || steps > r.max_steps || !valid_dtype(dtype))
    return APPNP_EINVAL;
  if (!(alpha >= 0.0f && alpha <= 1.0f) || (alpha == 0.0f && !r.alpha_zero)) return APPNP_EINVAL;
  if (!(p_drop >= 0.0f && p_drop < 1.0f)) return APPNP_EINVAL;
  if (g->row_lo != 0 || g->row_hi != g->n) return APPNP_EINVAL;  // needs the whole graph
  if (r.f32_only && dtype != APPNP_F32) return APPNP_ENOTSUP;
  if (r.undirected_only && !g->symmetric) return APPNP_ENOTSUP;
  if (r.transposed && needs_transpose(g) && !g->t_row_ptr) return APPNP_ENOTSUP;
  if (g->n == 0 || f == 0) return APPNP_OK;
  if (!in || !out || ld_in < f || ld_out < f || in == out || (r.has_extra && !r.extra))
    return APPNP_EINVAL;
  *run = 1;
  return APPNP_OK;
}

// the main part of the split (columns [0, fs)), 0 when there is no split or no main part
int64_t split_point(const appnp_graph* g, int64_t f, int dtype, bool aligned) {
  const int64_t r = remainder_cols(g, f, dtype, aligned);
  return r ? f - r : 0;
}

// The two split buffers of [n, f] fp32 rows with main part fs, back to back from a 256-B aligned
// base: each a main part [n, fs] and, 256-B aligned behind it, a remainder part [n, 4 rb_lpe]
// (fs = 0: narrow rows, all in the remainder pass).
struct SplitBufs {
  char* base;
  int64_t main_b, buf_b;  // bytes of a main part; of a whole buffer
  SplitBufs(const appnp_graph* g, int64_t n, int64_t fs, void* base_)
      : base(static_cast<char*>(base_)),
        main_b((n * fs * 4 + 255) / 256 * 256),
        buf_b((main_b + n * 16 * g->rb_lpe + 255) / 256 * 256) {}
  int64_t bytes() const { return 2 * buf_b; }
  float* main(int i) const { return reinterpret_cast<float*>(base + i * buf_b); }
  float* rem(int i) const { return reinterpret_cast<float*>(base + i * buf_b + main_b); }
};

// What both split loops begin with: `src` (H, or dZ) copied into split buffer 0, and the K
// remainder passes to come counted on the graph.
int split_copy_in(const appnp_graph* g, const void* src, int64_t ld, int64_t n, int64_t f,
                  int64_t fs, int K, const SplitBufs& b, hipStream_t s) {
  const int rc = timed(s, APPNP_KT_COPY, [&] {
    return launch_split_copy(static_cast<const float*>(src), ld, n, f, fs, 4 * g->rb_lpe,
                             b.main(0), b.rem(0), remainder_scale(g), s);
  });
  g->rem_launches.fetch_add(K, std::memory_order_relaxed);
  return rc;
}

// The forward loop in the split layout (appnp_blocks.hip).  Propagation is column-separable,
// so the main columns [0, fs) and the remainder columns [fs, f) are two independent K-step
// chains that meet only in Z:
//   * H is copied once into split buffer 0 (main part [n, fs], remainder part [n, 4]);
//   * main chain: K launches of the SpMM kernel on fs columns, gathering whole lines of the
//     main parts (ping-pong between the two buffers, the last into Z[:, :fs]);
//   * remainder chain: K persistent L2-resident passes over the remainder parts (the last
//     into Z[:, fs:f]).
// The chains touch disjoint parts of the buffers and disjoint columns of Z.  Both run on the
// caller's stream: on a side stream they overlapped in time but shared the memory system, and
// the total measured within 1 % of running them one after the other.
int propagate_split(const appnp_graph* g, const StepArgs& a0, const void* H, int64_t ld_h,
                    void* Z, int64_t ld_z, int64_t fs, int K, float p_drop, uint64_t seed,
                    const SplitBufs& b, hipStream_t s) {
  const int64_t f = a0.f;
  const int lpe = g->rb_lpe, rw = 4 * lpe;  // floats per remainder row
  const float* h = static_cast<const float*>(H);
  float* z = static_cast<float*>(Z);
  int rc = split_copy_in(g, H, ld_h, a0.n_rows, f, fs, K, b, s);
  StepArgs am = a0, ar = a0;  // main / remainder chain
  am.f = (int32_t)fs;
  am.h = H;
  am.ld_h = ld_h;
  am.ld_in = fs;
  int cur = 0;
  for (int k = 0; k < K && !rc; ++k) {
    const int dst = cur ^ 1;
    const bool last = k == K - 1;
    set_drop(am, p_drop, seed, k);
    am.zin = b.main(cur);
    am.out = last ? Z : b.main(dst);
    am.ld_out = last ? ld_z : fs;
    if (fs > 0) rc = timed_step(APPNP_F32, EPI_FWD, 4, am, s);
    if (rc) break;
    set_drop(ar, p_drop, seed, k);
    // LPE = 1: nv = 4 into the next remainder buffer (the shipped form); LPE > 1: nv is always
    // the valid remainder columns, to_rem says where the row goes
    const int nv = (lpe == 1 && !last) ? 4 : (int)(f - fs);
    rc = timed(s, APPNP_KT_REM, [&] {
      return launch_remainder(g, ar, EPI_FWD, b.rem(cur), h + fs, ld_h,
                              last ? z + fs : b.rem(dst), last ? ld_z : rw, nv, !last, s);
    });
    cur = dst;
  }
  return rc;
}

// The adjoint loop in the split layout: the same two independent chains as propagate_split,
// run backwards (G_K = dZ, G_k = (1-alpha) M_k^T G_{k+1}, dH += alpha' G_k), for a
// self-adjoint A_hat.  dH = alpha dZ is set by the caller.
int propagate_bwd_split(const appnp_graph* g, const StepArgs& a0, const void* dZ, int64_t ld_dz,
                        void* dH, int64_t ld_dh, int64_t fs, int K, float alpha, float p_drop,
                        uint64_t seed, const SplitBufs& b, hipStream_t s) {
  const int64_t f = a0.f;
  const int rw = 4 * g->rb_lpe;
  int rc = split_copy_in(g, dZ, ld_dz, a0.n_rows, f, fs, K, b, s);
  StepArgs am = a0, ar = a0;  // main / remainder chain
  am.f = (int32_t)fs;
  am.aux = dH;
  am.ld_aux = ld_dh;
  am.ld_in = fs;
  am.ld_out = fs;
  float* dh_rem = static_cast<float*>(dH) + fs;
  int cur = 0;
  for (int k = K - 1; k >= 0 && !rc; --k) {
    const int dst = cur ^ 1;
    const float a_k = k >= 1 ? alpha : 1.0f;
    set_drop(am, p_drop, seed, k);
    am.alpha = a_k;
    am.zin = b.main(cur);
    am.out = k == 0 ? nullptr : b.main(dst);
    if (fs > 0) rc = timed_step(APPNP_F32, EPI_BWD, 4, am, s);
    if (rc) break;
    set_drop(ar, p_drop, seed, k);
    ar.alpha = a_k;
    rc = timed(s, APPNP_KT_REM, [&] {
      return launch_remainder(g, ar, EPI_BWD, b.rem(cur), dh_rem, ld_dh,
                              k == 0 ? nullptr : b.rem(dst), rw, (int)(f - fs), true, s);
    });
    cur = dst;
  }
  return rc;
}

// ---- exact PPNP: Chebyshev semi-iteration on Z = (1-alpha) A_hat Z + alpha H ---------------

inline bool valid_solve_alpha(float alpha) { return alpha > 0.0f && alpha <= 1.0f; }

// w_{k+1} from w_k (k >= 1 steps done): w_1 = 1, w_2 = 1 / (1 - rho^2 / 2), then the recurrence
inline double next_omega(double rho, int k, double w) {
  return k == 0 ? 1.0 : k == 1 ? 1.0 / (1.0 - 0.5 * rho * rho) : 1.0 / (1.0 - 0.25 * rho * rho * w);
}

// What appnp_solve and appnp_plan_create_solve allow; the adjoint adds `transposed`
constexpr ChainRules kSolveRules = {1, kSolveMaxIters, false, true, true, false};

// `iters` steps from Z_0 = H on the CSR in `a`, the last into Z.  Step 1 is the plain forward
// step (w_1 = 1), step 2 reads Z_0 = H as its Z_{k-1}; from step 3 on Z_{k-1} sits in the
// workspace buffer the step overwrites (step k writes buffer (k-1) % 2, which holds Z_{k-2}), so
// two buffers carry the three-term recurrence.
int solve_loop(StepArgs a, const void* H, int64_t ld_h, void* Z, int64_t ld_z, int64_t f,
               int iters, float alpha, void* ws, size_t ws_bytes, hipStream_t s) {
  const int64_t ld_w = line_ld(f, APPNP_F32);
  const size_t buf_b = (size_t)(a.n_rows * ld_w * 4);
  Workspace w;  // iters = 2 needs one buffer, iters = 1 none
  const int rc = w.take(ws, ws_bytes, std::min(iters - 1, 2) * buf_b);
  if (rc) return rc;
  void* const buf[2] = {w.at(0), w.at(buf_b)};
  const int64_t lds[3] = {ld_h, ld_z, ld_w};
  const void* ptrs[4] = {H, Z, buf[0], buf[1]};
  const int V = pick_vec(APPNP_F32, f, lds, 3, ptrs, 4);
  a.h = H;
  a.ld_h = ld_h;
  const double rho = 1.0 - (double)alpha;
  double omega = 1.0;
  Chain c{H, ld_h};
  for (int k = 1; k <= iters; ++k) {
    omega = next_omega(rho, k - 1, omega);
    const bool last = k == iters;
    c.advance(a, last ? Z : buf[(k - 1) & 1], last ? ld_z : ld_w);
    int epi = EPI_FWD;
    if (k >= 2) {
      epi = EPI_CHEB;
      a.aux = k == 2 ? const_cast<void*>(H) : buf[(k - 1) & 1];
      a.ld_aux = k == 2 ? ld_h : ld_w;
      a.omega = (float)omega;
    }
    const int step_rc = timed_step(APPNP_F32, epi, V, a, s);
    if (step_rc) return step_rc;
  }
  return APPNP_OK;
}

// ---- polynomial propagation with device-resident coefficients ------------------------------
//
//   Z = sum_{k=0..K} gamma_k A_hat^k H
//
// Forward:  T_0 = H, T_k = A_hat T_{k-1}, Z accumulates gamma_k T_k: one launch of the step kernel
// per power (epilogue POLY: out = T_k, aux = Z); the first one also forms gamma_0 H.
// Backward, from <dZ, A_hat^k H> = <(A_hat^T)^k dZ, H>:  G_0 = dZ, G_k = A_hat^T G_{k-1},
// dH = sum_k gamma_k G_k, d gamma_k = <G_k, H>: the same launches on A_hat^T (aux = dH), whose
// epilogue POLY_DOT also leaves one fp32 partial of <G_k, H> per (column slab, row); a
// fixed-shape reduce sums them into dcoef[k].  No power of A_hat is stored or recomputed, and
// gamma is only ever read by the kernels, so a trainable gamma never crosses to the host.

// The workspace from its 256-B aligned base on: `bufs` ping-pong buffers of [n, ld_w] fp32 rows
// (the powers in flight), then the partial dots [slabs, n].  line_ld is not
// monotone in f (it pads rows only where that saves lines), so a buffer is sized for rows of
// whole lines, which bounds it and is.
struct PolyLayout {
  int bufs;
  int64_t ld_w;
  size_t buf_b, dots_at, bytes;
  PolyLayout(int64_t n, int64_t f, int K, bool with_dcoef)
      : bufs(std::min(std::max(K - 1, 0), 2)), ld_w(line_ld(f, APPNP_F32)),
        buf_b((size_t)n * round_up((size_t)f, 32) * 4), dots_at((size_t)bufs * buf_b),
        bytes(dots_at + (with_dcoef ? round_up((size_t)(poly_max_slabs(f) * n) * 4, 256) : 0)) {}
};

// K steps from `src` on the CSR of `a`: step k (1-based) gathers power k-1, writes power k into a
// workspace buffer (none for the last) and adds coef[k] times it to `acc`.  With `dots` every
// step also leaves the partials of <power k, a.h> there and a reduce sums them into dcoef[k].
// first_c0: step 1 starts `acc` from coef[0] * a.h (the forward, whose a.h is `src`).
int poly_steps(StepArgs a, const void* src, int64_t ld_src, void* acc, int64_t ld_acc, int K,
               const float* coef, bool first_c0, float* dots, float* dcoef, const PolyLayout& L,
               const Workspace& w, int V, hipStream_t s) {
  const int epi = dots ? EPI_POLY_DOT : EPI_POLY;
  a.aux = acc;
  a.ld_aux = ld_acc;
  a.dots = dots;
  Chain c{src, ld_src};
  for (int k = 1; k <= K; ++k) {
    c.advance(a, k == K ? nullptr : w.at((size_t)((k - 1) & 1) * L.buf_b), L.ld_w);
    a.coef = coef + k;
    a.coef0 = (first_c0 && k == 1) ? coef : nullptr;
    int64_t slabs = 0;
    int rc = timed(s, APPNP_KT_STEP,
                   [&] { return launch_step_slabs(APPNP_F32, epi, V, a, s, &slabs); });
    if (rc) return rc;
    if (dots) {
      rc = timed(s, APPNP_KT_COPY,
                 [&] { return launch_poly_reduce(dots, slabs * a.n_rows, dcoef + k, s); });
      if (rc) return rc;
    }
  }
  return APPNP_OK;
}

// ---- captured plans: the launches of appnp_propagate / appnp_solve replayed as one hipGraph --

}  // namespace

struct appnp_plan {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};

namespace {

// Capture what `enqueue(stream)` launches into a new plan.
template <typename Enqueue>
int plan_capture(Enqueue enqueue, appnp_plan** out) {
  if (!out) return APPNP_EINVAL;
  *out = nullptr;
  hipStream_t cs = nullptr;
  if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return APPNP_EDEVICE;
  appnp_plan* p = new (std::nothrow) appnp_plan();
  if (!p) {
    (void)hipStreamDestroy(cs);
    return APPNP_ENOMEM;
  }
  int rc = dev_err(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
  if (rc == APPNP_OK) {
    rc = enqueue(static_cast<void*>(cs));
    const hipError_t e = hipStreamEndCapture(cs, &p->graph);  // always end the capture
    if (rc == APPNP_OK) rc = dev_err(e);
  }
  if (rc == APPNP_OK) rc = dev_err(hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0));
  (void)hipStreamDestroy(cs);
  if (rc != APPNP_OK) {
    appnp_plan_destroy(p);
    return rc;
  }
  *out = p;
  return APPNP_OK;
}

}  // namespace

extern "C" {

size_t appnp_workspace_bytes(const appnp_graph* g, int64_t f, int64_t ld, int dtype) {
  if (!g || f < 0 || !valid_dtype(dtype)) return 0;
  (void)ld;  // the workspace uses its own line-aligned leading dimension
  const int64_t rows = g->row_hi - g->row_lo;
  // two ping-pong buffers (the forward needs one, the adjoint two), 256-B aligned each
  int64_t need = 2 * rows * line_ld(f, dtype) * elem_size(dtype) + 2048;
  // the split layout: two buffers [n, fs] + [n, 4 rb_lpe] (a W8 / W16 remainder row is wider
  // than the packed row's tail), plus the alignment of the base
  const int64_t r = (g->row_lo == 0 && g->row_hi == g->n) ? remainder_cols(g, f, dtype, true) : 0;
  if (r > 0) need = std::max<int64_t>(need, SplitBufs(g, rows, f - r, nullptr).bytes() + 256);
  return (size_t)need;
}

int appnp_propagate_split_point(const appnp_graph* g, int64_t f, int dtype, int64_t* fs) {
  if (!g || !fs || f < 0 || !valid_dtype(dtype)) return APPNP_EINVAL;
  *fs = split_point(g, f, dtype, true);
  return APPNP_OK;
}

int appnp_propagate_remainder_cols(const appnp_graph* g, int64_t f, int dtype, int64_t* r) {
  if (!g || !r || f < 0 || !valid_dtype(dtype)) return APPNP_EINVAL;
  *r = remainder_cols(g, f, dtype, true);
  return APPNP_OK;
}

int appnp_propagate(const appnp_graph* g, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
                    int64_t f, int dtype, int K, float alpha, float p_drop, uint64_t seed,
                    void* ws, size_t ws_bytes, void* stream) {
  int run = 0;
  int rc = check_chain(g, H, ld_h, Z, ld_z, f, dtype, K, alpha, p_drop,
                       {0, INT_MAX, true, false, false, false}, &run);
  if (rc || !run) return rc;
  const int64_t n = g->n;
  const hipStream_t s = as_stream(stream);
  const int64_t es = elem_size(dtype);
  if (K == 0)
    return timed(s, APPNP_KT_COPY, [&] {
      return hipMemcpy2DAsync(Z, ld_z * es, H, ld_h * es, f * es, n, hipMemcpyDeviceToDevice, s);
    });
  // Z and one workspace buffer alternate (K = 1 needs none)
  const int64_t ld_w = line_ld(f, dtype);
  Workspace w;
  rc = w.take(ws, ws_bytes, std::min(K - 1, 1) * (size_t)(n * ld_w * es));
  if (rc) return rc;
  void* const buf = w.at(0);
  const int64_t lds[3] = {ld_h, ld_z, ld_w};
  const void* ptrs[3] = {H, Z, buf};
  const int V = pick_vec(dtype, f, lds, 3, ptrs, 3);

  StepArgs a = base_args(g, f, alpha);
  a.h = H;
  a.ld_h = ld_h;
  const int64_t hz_lds[2] = {ld_h, ld_z};
  const void* hz[2] = {H, Z};
  const int64_t r = K >= 2 ? remainder_cols(g, f, dtype, vec16(hz_lds, 2, hz, 2)) : 0;
  if (r > 0) {
    // the split buffers take the place of the ping-pong buffer, where the workspace holds them
    const SplitBufs b(g, n, f - r, buf);
    if (w.room >= (size_t)b.bytes())
      return propagate_split(g, a, H, ld_h, Z, ld_z, f - r, K, p_drop, seed, b, s);
  }
  Chain c{H, ld_h};
  for (int k = 0; k < K; ++k) {
    // the last iteration must land in Z: alternate backwards from it
    const bool to_z = ((K - 1 - k) % 2) == 0;
    c.advance(a, to_z ? Z : buf, to_z ? ld_z : ld_w);
    set_drop(a, p_drop, seed, k);
    rc = timed_step(dtype, EPI_FWD, V, a, s);
    if (rc) return rc;
  }
  return APPNP_OK;
}

int appnp_propagate_bwd(const appnp_graph* g, const void* dZ, int64_t ld_dz, void* dH,
                        int64_t ld_dh, int64_t f, int dtype, int K, float alpha, float p_drop,
                        uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
  // A_hat^T: A_hat itself for 'sym' on an undirected graph, else the transposed CSR built at
  // creation (APPNP_GRAPH_TRANSPOSE)
  int run = 0;
  int rc = check_chain(g, dZ, ld_dz, dH, ld_dh, f, dtype, K, alpha, p_drop,
                       {0, INT_MAX, true, false, false, true}, &run);
  if (rc || !run) return rc;
  const int64_t n = g->n;
  const hipStream_t s = as_stream(stream);
  const int64_t es = elem_size(dtype);
  if (K == 0)
    return timed(s, APPNP_KT_COPY, [&] {
      return hipMemcpy2DAsync(dH, ld_dh * es, dZ, ld_dz * es, f * es, n, hipMemcpyDeviceToDevice,
                              s);
    });
  // G_{K-1} .. G_1 alternate between two workspace buffers (K = 2 needs one, K = 1 none)
  const int64_t ld_w = line_ld(f, dtype);
  const size_t buf_b = (size_t)(n * ld_w * es);
  Workspace w;
  rc = w.take(ws, ws_bytes, std::min(K - 1, 2) * buf_b);
  if (rc) return rc;
  void* const buf[2] = {w.at(0), w.at(buf_b)};
  const int64_t lds[3] = {ld_dz, ld_dh, ld_w};
  // at K = 1 the workspace pointer counts as the caller gave it, though no step touches it
  const void* ptrs[4] = {dZ, dH, K == 1 ? ws : buf[0], buf[1]};
  const int V = pick_vec(dtype, f, lds, 3, ptrs, 4);

  // dH = alpha * dZ  (the k = K term), then G_k = (1-alpha) M_k^T G_{k+1},
  // dH += alpha G_k (k >= 1) / dH += G_0.
  rc = timed(s, APPNP_KT_COPY,
             [&] { return launch_scale_rows(dtype, dZ, ld_dz, dH, ld_dh, n, f, alpha, s); });
  if (rc) return rc;
  // split rows (self-adjoint A_hat: the source-blocked copy of A_hat is that of A_hat^T)
  const int64_t dd_lds[2] = {ld_dz, ld_dh};
  const void* dd[2] = {dZ, dH};
  const int64_t r = (!needs_transpose(g) && K >= 2)
                        ? remainder_cols(g, f, dtype, vec16(dd_lds, 2, dd, 2)) : 0;
  StepArgs a = base_args(g, f, alpha);
  if (needs_transpose(g)) use_transpose(a, g);
  a.tkey = 1;  // entry (j, i) of A_hat^T carries the mask of forward edge (i, j)
  if (r > 0) {
    const SplitBufs b(g, n, f - r, buf[0]);
    if (w.room >= (size_t)b.bytes())  // else too small: whole rows
      return propagate_bwd_split(g, a, dZ, ld_dz, dH, ld_dh, f - r, K, alpha, p_drop, seed, b, s);
  }
  a.aux = dH;
  a.ld_aux = ld_dh;
  Chain c{dZ, ld_dz};
  int flip = 0;
  for (int k = K - 1; k >= 0; --k) {
    c.advance(a, k == 0 ? nullptr : buf[flip], ld_w);
    a.alpha = k >= 1 ? alpha : 1.0f;
    set_drop(a, p_drop, seed, k);
    rc = timed_step(dtype, EPI_BWD, V, a, s);
    if (rc) return rc;
    flip ^= 1;
  }
  return APPNP_OK;
}

int appnp_solve_iterations(float alpha, float tol, int* iters) {
  if (!iters || !valid_solve_alpha(alpha) || !(tol > 0.0f && tol < 1.0f)) return APPNP_EINVAL;
  const double rho = 1.0 - (double)alpha;
  const double sigma = rho / (1.0 + std::sqrt(1.0 - rho * rho));
  double p = 1.0;  // sigma^m
  for (int m = 1; m <= kSolveMaxIters; ++m) {
    p *= sigma;
    if (2.0 * p / (1.0 + p * p) <= (double)tol) {
      *iters = m;
      return APPNP_OK;
    }
  }
  return APPNP_ERANGE;
}

int appnp_solve_weights(float alpha, int iters, double* omega) {
  if (!omega || !valid_solve_alpha(alpha) || iters < 1 || iters > kSolveMaxIters)
    return APPNP_EINVAL;
  const double rho = 1.0 - (double)alpha;
  double w = 1.0;
  for (int k = 0; k < iters; ++k) omega[k] = w = next_omega(rho, k, w);
  return APPNP_OK;
}

int appnp_solve(const appnp_graph* g, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
                int64_t f, int dtype, int iters, float alpha, void* ws, size_t ws_bytes,
                void* stream) {
  int run = 0;
  const int rc = check_chain(g, H, ld_h, Z, ld_z, f, dtype, iters, alpha, 0.0f, kSolveRules, &run);
  if (rc || !run) return rc;
  // whole rows, also on a graph with a source-blocked copy: no split layout, no remainder pass
  return solve_loop(base_args(g, f, alpha), H, ld_h, Z, ld_z, f, iters, alpha, ws, ws_bytes,
                    as_stream(stream));
}

int appnp_solve_bwd(const appnp_graph* g, const void* dZ, int64_t ld_dz, void* dH, int64_t ld_dh,
                    int64_t f, int dtype, int iters, float alpha, void* ws, size_t ws_bytes,
                    void* stream) {
  ChainRules rules = kSolveRules;
  rules.transposed = true;
  int run = 0;
  const int rc = check_chain(g, dZ, ld_dz, dH, ld_dh, f, dtype, iters, alpha, 0.0f, rules, &run);
  if (rc || !run) return rc;
  // Pi^T = alpha (I - (1-alpha) A_hat^T)^-1: the same solve on A_hat^T, whose spectrum is A_hat's
  StepArgs a = base_args(g, f, alpha);
  // the graph is undirected here, so needs_transpose(g) is mode != APPNP_NORM_SYM
  if (needs_transpose(g)) use_transpose(a, g);
  return solve_loop(a, dZ, ld_dz, dH, ld_dh, f, iters, alpha, ws, ws_bytes, as_stream(stream));
}

size_t appnp_poly_workspace_bytes(const appnp_graph* g, int64_t f, int K, int with_dcoef) {
  if (!g || f <= 0 || f > INT32_MAX || K < 0 || K > kPolyMaxK) return 0;
  const int64_t n = g->row_hi - g->row_lo;
  if (n <= 0) return 0;
  const size_t need = PolyLayout(n, f, K, with_dcoef != 0).bytes;
  return need ? need + 256 : 0;  // the alignment of the base
}

int appnp_poly(const appnp_graph* g, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
               int64_t f, int dtype, int K, const float* coef, void* ws, size_t ws_bytes,
               void* stream) {
  int run = 0;
  const int rc = check_chain(g, H, ld_h, Z, ld_z, f, dtype, K, 0.0f, 0.0f,
                             {0, kPolyMaxK, true, true, false, false, true, coef}, &run);
  if (rc || !run) return rc;
  const int64_t n = g->n;
  const PolyLayout L(n, f, K, false);
  Workspace w;
  if (w.take(ws, ws_bytes, L.bytes)) return APPNP_EINVAL;
  const hipStream_t s = as_stream(stream);
  const float* h = static_cast<const float*>(H);
  float* z = static_cast<float*>(Z);
  if (K == 0)  // Z = gamma_0 H
    return timed(s, APPNP_KT_COPY, [&] {
      return launch_poly_rows(h, ld_h, z, ld_z, nullptr, 0, nullptr, n, f, coef, s);
    });
  const int64_t lds[3] = {ld_h, ld_z, L.ld_w};
  const void* ptrs[3] = {H, Z, L.bufs ? w.at(0) : nullptr};
  const int V = pick_vec(APPNP_F32, f, lds, 3, ptrs, 3);
  // whole rows, also on a graph with a source-blocked copy: no split layout, no remainder pass
  StepArgs a = base_args(g, f, 0.0f);
  a.h = H;
  a.ld_h = ld_h;
  return poly_steps(a, H, ld_h, Z, ld_z, K, coef, true, nullptr, nullptr, L, w, V, s);
}

int appnp_poly_bwd(const appnp_graph* g, const void* dZ, int64_t ld_dz, const void* H,
                   int64_t ld_h, void* dH, int64_t ld_dh, float* dcoef, int64_t f, int dtype,
                   int K, const float* coef, void* ws, size_t ws_bytes, void* stream) {
  int run = 0;
  const int rc = check_chain(g, dZ, ld_dz, dH, ld_dh, f, dtype, K, 0.0f, 0.0f,
                             {0, kPolyMaxK, true, true, false, true, true, coef}, &run);
  if (rc || !run) return rc;
  if (dcoef && (!H || ld_h < f || H == dH)) return APPNP_EINVAL;
  const int64_t n = g->n;
  const PolyLayout L(n, f, K, dcoef != nullptr);
  Workspace w;
  if (w.take(ws, ws_bytes, L.bytes)) return APPNP_EINVAL;
  const hipStream_t s = as_stream(stream);
  float* dots = dcoef ? static_cast<float*>(w.at(L.dots_at)) : nullptr;
  if (!dcoef) {
    H = nullptr;
    ld_h = 0;
  }
  // dH = gamma_0 dZ and d gamma_0 = <dZ, H>
  int irc = timed(s, APPNP_KT_COPY, [&] {
    return launch_poly_rows(static_cast<const float*>(dZ), ld_dz, static_cast<float*>(dH), ld_dh,
                            static_cast<const float*>(H), ld_h, dots, n, f, coef, s);
  });
  if (irc) return irc;
  if (dcoef) {
    irc = timed(s, APPNP_KT_COPY, [&] { return launch_poly_reduce(dots, n, dcoef, s); });
    if (irc) return irc;
  }
  if (K == 0) return APPNP_OK;
  const int64_t lds[4] = {ld_dz, ld_dh, L.ld_w, dcoef ? ld_h : L.ld_w};
  const void* ptrs[4] = {dZ, dH, L.bufs ? w.at(0) : nullptr, H};
  const int V = pick_vec(APPNP_F32, f, lds, 4, ptrs, 4);
  StepArgs a = base_args(g, f, 0.0f);
  if (needs_transpose(g)) use_transpose(a, g);
  a.h = H;
  a.ld_h = ld_h;
  return poly_steps(a, dZ, ld_dz, dH, ld_dh, K, coef, false, dots, dcoef, L, w, V, s);
}

int appnp_plan_create(const appnp_graph* g, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
                      int64_t f, int dtype, int K, float alpha, float p_drop, uint64_t seed,
                      void* ws, size_t ws_bytes, appnp_plan** out) {
  return plan_capture(
      [&](void* cs) {
        return appnp_propagate(g, H, ld_h, Z, ld_z, f, dtype, K, alpha, p_drop, seed, ws,
                               ws_bytes, cs);
      },
      out);
}

int appnp_plan_create_solve(const appnp_graph* g, const void* H, int64_t ld_h, void* Z,
                            int64_t ld_z, int64_t f, int dtype, int iters, float alpha, void* ws,
                            size_t ws_bytes, appnp_plan** out) {
  if (!out) return APPNP_EINVAL;
  *out = nullptr;
  int run = 0;  // bad arguments fail here, before the capture stream is created
  const int rc = check_chain(g, H, ld_h, Z, ld_z, f, dtype, iters, alpha, 0.0f, kSolveRules, &run);
  if (rc) return rc;
  return plan_capture(
      [&](void* cs) {
        return appnp_solve(g, H, ld_h, Z, ld_z, f, dtype, iters, alpha, ws, ws_bytes, cs);
      },
      out);
}

int appnp_plan_launch(const appnp_plan* p, void* stream) {
  if (!p || !p->exec) return APPNP_EINVAL;
  return dev_err(hipGraphLaunch(p->exec, as_stream(stream)));
}

void appnp_plan_destroy(appnp_plan* p) {
  if (!p) return;
  if (p->exec) (void)hipGraphExecDestroy(p->exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  delete p;
}

}  // extern "C"
