// appnp_poly.hip -- polynomial propagation with device-resident coefficients (appnp_poly*).
//
//   Z = sum_{k=0..K} gamma_k A_hat^k H
//
// Forward:  T_0 = H, T_k = A_hat T_{k-1}, Z accumulates gamma_k T_k: one launch of the step kernel
// per power (epilogue POLY: out = T_k, aux = Z); the first one also forms gamma_0 H.
// Backward, from <dZ, A_hat^k H> = <(A_hat^T)^k dZ, H>:  G_0 = dZ, G_k = A_hat^T G_{k-1},
// dH = sum_k gamma_k G_k, d gamma_k = <G_k, H>: the same launches on A_hat^T (aux = dH), whose
// epilogue POLY_DOT also leaves one fp32 partial of <G_k, H> per (column slab, row); a
// fixed-shape reduce sums them into dcoef[k].  No power of A_hat is stored or recomputed.
//
// This unit holds no kernel (they are appnp_spmm.hip's): argument checks, the workspace and the
// launch sequence.  Nothing here synchronises or allocates, and gamma is only ever read by the
// kernels, so both calls can be captured and a trainable gamma never crosses to the host.
#include <algorithm>

#include "../../include/ppnp_amd.h"
#include "appnp_internal.h"

namespace {

using appnp::StepArgs;
using appnp::as_stream;
using appnp::line_ld;
using appnp::round_up;
using appnp::timed;

constexpr int kPolyMaxK = APPNP_POLY_MAX_K;

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
        bytes(dots_at +
              (with_dcoef ? round_up((size_t)(appnp::poly_max_slabs(f) * n) * 4, 256) : 0)) {}
};

// Argument checks of appnp_poly / appnp_poly_bwd in the order of appnp_solve's, before any
// device call.  *run = 0: valid and nothing to do (an empty graph or F = 0).
int check_poly(const appnp_graph* g, const void* in, int64_t ld_in, const void* out,
               int64_t ld_out, int64_t f, int dtype, int K, const float* coef, bool transposed,
               int* run) {
  *run = 0;
  if (!g) return APPNP_EINVAL;
  if (f < 0 || f > INT32_MAX || K < 0 || K > kPolyMaxK ||
      (dtype != APPNP_F32 && dtype != APPNP_BF16))
    return APPNP_EINVAL;
  if (g->row_lo != 0 || g->row_hi != g->n) return APPNP_EINVAL;  // needs the whole graph
  if (dtype != APPNP_F32) return APPNP_ENOTSUP;
  const bool self_adjoint = g->mode == APPNP_NORM_SYM && g->symmetric;
  if (transposed && !self_adjoint && !g->t_row_ptr) return APPNP_ENOTSUP;
  if (g->n == 0 || f == 0) return APPNP_OK;
  if (!in || !out || ld_in < f || ld_out < f || in == out || !coef) return APPNP_EINVAL;
  *run = 1;
  return APPNP_OK;
}

// The aligned base of the caller's workspace, or null when it cannot hold `need` bytes from there.
char* workspace_base(void* ws, size_t ws_bytes, size_t need) {
  if (need == 0) return reinterpret_cast<char*>(uintptr_t(256));  // never dereferenced
  if (!ws) return nullptr;
  const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
  const uintptr_t aligned = (base + 255) & ~uintptr_t(255);
  if (ws_bytes < need + (aligned - base)) return nullptr;
  return reinterpret_cast<char*>(aligned);
}

// K steps from `src` on the CSR of `a`: step k (1-based) gathers power k-1, writes power k into a
// workspace buffer (none for the last) and adds coef[k] times it to `acc`.  With `dots` every
// step also leaves the partials of <power k, a.h> there and a reduce sums them into dcoef[k].
// first_c0: step 1 starts `acc` from coef[0] * a.h (the forward, whose a.h is `src`).
int poly_steps(StepArgs a, const void* src, int64_t ld_src, void* acc, int64_t ld_acc, int K,
               const float* coef, bool first_c0, float* dots, float* dcoef, const PolyLayout& L,
               char* base, int V, hipStream_t s) {
  const int epi = dots ? appnp::EPI_POLY_DOT : appnp::EPI_POLY;
  a.aux = acc;
  a.ld_aux = ld_acc;
  a.dots = dots;
  a.ld_out = L.ld_w;
  const void* zin = src;
  int64_t ld_in = ld_src;
  for (int k = 1; k <= K; ++k) {
    a.zin = zin;
    a.ld_in = ld_in;
    a.out = k == K ? nullptr : base + (size_t)((k - 1) & 1) * L.buf_b;
    a.coef = coef + k;
    a.coef0 = (first_c0 && k == 1) ? coef : nullptr;
    int64_t slabs = 0;
    int rc = timed(s, APPNP_KT_STEP, [&] {
      return appnp::launch_step_slabs(APPNP_F32, epi, V, a, s, &slabs);
    });
    if (rc) return rc;
    if (dots) {
      rc = timed(s, APPNP_KT_COPY, [&] {
        return appnp::launch_poly_reduce(dots, slabs * a.n_rows, dcoef + k, s);
      });
      if (rc) return rc;
    }
    zin = a.out;
    ld_in = L.ld_w;
  }
  return APPNP_OK;
}

}  // namespace

extern "C" {

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
  const int rc = check_poly(g, H, ld_h, Z, ld_z, f, dtype, K, coef, false, &run);
  if (rc || !run) return rc;
  const int64_t n = g->n;
  const PolyLayout L(n, f, K, false);
  char* base = workspace_base(ws, ws_bytes, L.bytes);
  if (!base) return APPNP_EINVAL;
  const hipStream_t s = as_stream(stream);
  const float* h = static_cast<const float*>(H);
  float* z = static_cast<float*>(Z);
  if (K == 0)  // Z = gamma_0 H
    return timed(s, APPNP_KT_COPY, [&] {
      return appnp::launch_poly_rows(h, ld_h, z, ld_z, nullptr, 0, nullptr, n, f, coef, s);
    });
  const int64_t lds[3] = {ld_h, ld_z, L.ld_w};
  const void* ptrs[3] = {H, Z, L.bufs ? base : nullptr};
  const int V = appnp::pick_vec(APPNP_F32, f, lds, 3, ptrs, 3);
  // whole rows, also on a graph with a source-blocked copy: no split layout, no remainder pass
  StepArgs a = appnp::base_args(g, f, 0.0f);
  a.h = H;
  a.ld_h = ld_h;
  return poly_steps(a, H, ld_h, Z, ld_z, K, coef, true, nullptr, nullptr, L, base, V, s);
}

int appnp_poly_bwd(const appnp_graph* g, const void* dZ, int64_t ld_dz, const void* H,
                   int64_t ld_h, void* dH, int64_t ld_dh, float* dcoef, int64_t f, int dtype,
                   int K, const float* coef, void* ws, size_t ws_bytes, void* stream) {
  int run = 0;
  const int rc = check_poly(g, dZ, ld_dz, dH, ld_dh, f, dtype, K, coef, true, &run);
  if (rc || !run) return rc;
  if (dcoef && (!H || ld_h < f || H == dH)) return APPNP_EINVAL;
  const int64_t n = g->n;
  const PolyLayout L(n, f, K, dcoef != nullptr);
  char* base = workspace_base(ws, ws_bytes, L.bytes);
  if (!base) return APPNP_EINVAL;
  const hipStream_t s = as_stream(stream);
  float* dots = dcoef ? reinterpret_cast<float*>(base + L.dots_at) : nullptr;
  if (!dcoef) {
    H = nullptr;
    ld_h = 0;
  }
  // dH = gamma_0 dZ and d gamma_0 = <dZ, H>
  int irc = timed(s, APPNP_KT_COPY, [&] {
    return appnp::launch_poly_rows(static_cast<const float*>(dZ), ld_dz, static_cast<float*>(dH),
                                   ld_dh, static_cast<const float*>(H), ld_h, dots, n, f, coef, s);
  });
  if (irc) return irc;
  if (dcoef) {
    irc = timed(s, APPNP_KT_COPY, [&] { return appnp::launch_poly_reduce(dots, n, dcoef, s); });
    if (irc) return irc;
  }
  if (K == 0) return APPNP_OK;
  const int64_t lds[4] = {ld_dz, ld_dh, L.ld_w, dcoef ? ld_h : L.ld_w};
  const void* ptrs[4] = {dZ, dH, L.bufs ? base : nullptr, H};
  const int V = appnp::pick_vec(APPNP_F32, f, lds, 4, ptrs, 4);
  StepArgs a = appnp::base_args(g, f, 0.0f);
  if (!(g->mode == APPNP_NORM_SYM && g->symmetric)) appnp::use_transpose(a, g);
  a.h = H;
  a.ld_h = ld_h;
  return poly_steps(a, dZ, ld_dz, dH, ld_dh, K, coef, false, dots, dcoef, L, base, V, s);
}

}  // extern "C"
