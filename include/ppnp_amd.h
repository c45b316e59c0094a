/*
 * ppnp_amd.h -- C ABI of the MI355X (gfx950) APPNP propagation path.
 *
 * This is the drop-in boundary for the propagation hot path of bkj/ppnp.  The reference
 * has no FFI of its own (it is pure Python); each entry point below names the reference
 * interface it replaces (file:line under the reference checkout):
 *
 *   appnp_graph_create*   helpers.py:58-66   calc_A_hat(adj, mode)   (host scipy, fp64)
 *                         helpers.py:68-71   compute_ppr(...)         (dense O(N^3) inverse)
 *   appnp_propagate       model.py:63        self.ppr[idx] @ self.encoder(X)  -- the dense
 *                                            PPR product becomes K fused CSR SpMM+AXPBY
 *                                            launches  Z <- (1-a) A_hat Z + a H
 *   appnp_propagate_bwd   model.py:63        autograd of the same product (dH = J^T dZ)
 *   appnp_step            one iteration; used by the row-partitioned multi-GPU driver
 *   appnp_step_split      the same on the split layout (whole-line main columns + the
 *                         L2-blocked remainder pass) of a row-partitioned graph
 *   appnp_dist_*          the row partition's whole K loop (SURVEY.md 8(b) appnp_dist_create)
 *   appnp_standardize     ppnp/data/sparsegraph.py:191-222  SparseGraph.standardize
 *                         (unweighted, undirected, no self loops, largest CC)
 *   appnp_spmm            model.py:36-38,47  Dropout + X @ W1 of the encoder on a CSR X
 *                         (main.py:91 densifies X; 1.76 % dense on Cora-ML)
 *
 * Conventions
 *   - Every function returns 0 (APPNP_OK) or a negative errno-style code; nothing throws or
 *     aborts across the ABI.  appnp_strerror() names a code.
 *   - All array arguments are DEVICE pointers on the current HIP device; the caller owns H,
 *     Z, dZ, dH and the workspace; the graph handle owns its device CSR.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  appnp_propagate,
 *     appnp_propagate_bwd and appnp_step are asynchronous and stream-ordered: no host sync,
 *     no allocation (graph-capturable).  appnp_graph_create* allocates and synchronises.
 *   - Dense matrices are row-major with a leading dimension `ld` in ELEMENTS (ld >= f).
 *   - A handle is not thread-safe; distinct handles are independent.
 */
#ifndef PPNP_AMD_H
#define PPNP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): appnp_dist_workspace_bytes reserves staging for a misaligned H / Z (a larger
 * workspace than version 1 asked for); the pipelined row steps (appnp_graph_shard_offsets,
 * appnp_step_shards, appnp_step_split_shards, appnp_dist_set_broadcast); the per-launch timer
 * brackets each launch (start and end events) and has the kinds APPNP_KT_LOCAL / _REMOTE /
 * _XCHG; appnp_tuning_overrides / appnp_tuning_names.
 * Added since, backward compatible (the version stays 2): the exact PPNP solver
 * appnp_solve_iterations, appnp_solve_weights, appnp_solve, appnp_solve_bwd and
 * appnp_plan_create_solve; the column top-k selection appnp_topk_workspace_bytes and
 * appnp_topk_columns; PPR columns by forward push, appnp_push_workspace_bytes and
 * appnp_push_columns, with the timer kind APPNP_KT_PUSH; the top k straight from the push,
 * appnp_push_topk_workspace_bytes and appnp_push_topk; the per-minibatch slice of a sparse PPR
 * matrix with its transpose, appnp_csr_batch_workspace_bytes, appnp_csr_batch_count and
 * appnp_csr_batch_emit; whole rows of a device CSR with the transpose of the slice,
 * appnp_csr_rows_workspace_bytes, appnp_csr_rows_count and appnp_csr_rows_emit; polynomial
 * propagation with coefficients in device memory, appnp_poly_workspace_bytes, appnp_poly and
 * appnp_poly_bwd. */
#define PPNP_AMD_ABI_VERSION 2

typedef struct appnp_graph appnp_graph;

enum appnp_status {
  APPNP_OK = 0,
  APPNP_EDEVICE = -5,   /* HIP runtime / kernel launch failure            */
  APPNP_ENOMEM = -12,   /* device allocation failed                       */
  APPNP_EINVAL = -22,   /* bad argument (shape, pointer, ld, alignment)   */
  APPNP_ERANGE = -34,   /* size exceeds the int32 CSR index range         */
  APPNP_ENOTSUP = -95   /* valid request this build does not implement    */
};

/* helpers.py:61-66: 'sym' = D^-1/2 (A+I) D^-1/2, 'rw' = D^-1 (A+I) */
enum appnp_norm { APPNP_NORM_SYM = 0, APPNP_NORM_RW = 1 };

/* OR into `mode` of appnp_graph_create: also build A_hat^T (full graphs only) so that
 * appnp_propagate_bwd works for 'rw' and for directed graphs.  Not needed (and not built)
 * for 'sym' on an undirected graph, where A_hat^T == A_hat. */
#define APPNP_GRAPH_TRANSPOSE 0x100

/* OR into `mode`: also keep a copy of A_hat regrouped by source block (2^15 source rows per
 * block; full graphs only).  appnp_propagate then takes the last 1-4 columns of fp32 rows
 * with F = 32q + r (e.g. F = 100) out of the random gather and forms their product in one
 * persistent, L2-resident pass per iteration, so a gathered row costs q cache lines instead
 * of q + 1.  Costs 8 bytes per nonzero (4 on an unweighted graph without self loops, whose
 * entries need no values, plus 8 bytes per node) plus one int32 per (block, 640-row group) of
 * device memory (segments padded to 64 entries).  Best-effort: when the copy cannot be built (too many blocks, device memory), the
 * graph is still created and gathers whole rows; appnp_graph_source_blocks tells. */
#define APPNP_GRAPH_SOURCE_BLOCKS 0x200

/* OR into `mode` instead of (or with) APPNP_GRAPH_SOURCE_BLOCKS: the source-blocked copy for a
 * remainder of up to 8 (W8) or 16 (W16) columns: fp32 rows of F = 32q + r features with
 * r <= 8 on a W8 copy (a wider remainder beside a main part costs as much as its extra line,
 * measured), and narrow rows F <= 8 / 16 whole (for example F = 40 = 32 + 8, or the 12-13-column
 * slabs of an 8-rank column layout of F = 100).  A W16 copy serves narrow rows only: beside a
 * main part its 4 row passes cost more than the extra line (F = 100 / 36 measured), so such
 * rows stay whole on it.  The pass then gives 2 / 4 lanes to each
 * entry and holds 320 / 160 rows per wave group, so a graph may need 2 / 4 row passes per
 * launch.  Same memory as APPNP_GRAPH_SOURCE_BLOCKS (segments padded to 32 / 16 entries). */
#define APPNP_GRAPH_SB_W8 0x400
#define APPNP_GRAPH_SB_W16 0x800

/* storage type of H / Z (accumulation is always fp32) */
enum appnp_dtype { APPNP_F32 = 0, APPNP_BF16 = 1 };

int appnp_abi_version(void);
/* Provenance of this build: "src=<digest of the .hip and .h files of ppnp_amd/csrc and of this
 * header (srcdigest.py)>;abi=..;arch=<the Makefile's ARCH, gfx950>;compiler=..;built=..".
 * bench.py prints it next to the digest of the tree it runs in, so a library built from other
 * sources shows. */
const char* appnp_build_info(void);
const char* appnp_strerror(int code);

/*
 * Build A_hat on the device from the CSR of A (helpers.py:58-66).
 *   indptr[n+1], indices[nnz]: int32 CSR of A, columns strictly increasing in each row
 *                              (scipy canonical form); device pointers.
 *   vals[nnz]: fp32 edge weights, or NULL for an unweighted graph (all ones).
 *   A may or may not contain diagonal entries: A+I merges them (a_ii + 1), exactly as
 *   `adj + sp.eye(n)` does, and entries whose merged value is 0 are dropped.
 * Degrees are fp64 weighted row sums of A+I; A_hat values are computed in fp64 and rounded
 * once to fp32, so they equal float32(calc_A_hat(adj, mode).data) bit for bit.
 */
int appnp_graph_create(const int32_t* indptr, const int32_t* indices, const float* vals,
                       int64_t n, int64_t nnz, int mode, void* stream, appnp_graph** out);

/*
 * Device-side SparseGraph.standardize (ppnp/data/sparsegraph.py:191-222): unweighted,
 * undirected (pattern of A + A^T), no self loops and, if select_lcc, only the largest
 * connected component with nodes renumbered in increasing order (create_subgraph,
 * sparsegraph.py:300-352).  Input: CSR of the raw adjacency (device; vals may be NULL;
 * explicit zero weights count as absent).  Output: a handle owning the standardized int32
 * CSR (sorted columns) and node_map[n_out] (int64 input node id of each kept node), which
 * subsets attributes/labels exactly as the reference does.  Allocates and synchronises.
 * Ties for the largest component go to the one with the largest smallest node index (the
 * reference's np.argsort(sizes)[::-1][:1] is not stable, so its own tie order depends on the
 * numpy build; real datasets have a unique largest component).
 */
typedef struct appnp_csr appnp_csr;
int appnp_standardize(const int32_t* indptr, const int32_t* indices, const float* vals,
                      int64_t n, int64_t nnz, int select_lcc, void* stream, appnp_csr** out);
int appnp_csr_info(const appnp_csr* c, int64_t* n, int64_t* nnz, int64_t* n_in);
int appnp_csr_copy(const appnp_csr* c, int32_t* indptr, int32_t* indices, int64_t* node_map,
                   void* stream);
void appnp_csr_destroy(appnp_csr* c);

/* Transpose of a CSR (rows x cols) as a canonical CSR (cols x rows, columns = input rows in
 * increasing order), values carried when vals != NULL.  appnp_csr_info reports n = cols,
 * n_in = rows; appnp_csr_copy gives indptr/indices (node_map unused); appnp_csr_values the
 * values.  Allocates and synchronises. */
int appnp_csr_transpose(const int32_t* indptr, const int32_t* indices, const float* vals,
                        int64_t rows, int64_t cols, int64_t nnz, void* stream, appnp_csr** out);
int appnp_csr_values(const appnp_csr* c, float* data, void* stream);

/*
 * General sparse x dense product on the same fused kernel family (fp32):
 *   C[rows, f] = (M o A) B,   A: CSR rows x cols (vals NULL = all ones), B: cols x f (ld_b)
 * with optional entry dropout M (keep iff 24-bit hash of (seed, 0, i, j) >= p * 2^24, kept
 * entries scaled by 1/(1-p)); transposed_key != 0 keys entry (i, j) as (j, i), so the product
 * with A^T (appnp_csr_transpose) replays the mask of A -- the backward of a dropout SpMM.
 * Used for the sparse encoder input (model.py:36-38, 47 on a CSR X; main.py:91 densifies X).
 */
int appnp_spmm(const int32_t* indptr, const int32_t* indices, const float* vals, int64_t rows,
               int64_t cols, const float* B, int64_t ld_b, float* C, int64_t ld_c, int64_t f,
               float p_drop, uint64_t seed, int transposed_key, void* stream);

/*
 * Same as appnp_graph_create, but keeps only rows [row_lo, row_hi) of A_hat (global column indices); degrees of
 * all n nodes are still computed from the full A.  Used for the row-partitioned multi-GPU
 * path: rank r owns rows [row_lo, row_hi).  With split_local != 0 the rows are also stored
 * as two CSRs -- columns inside [row_lo,row_hi) ("local") and outside ("remote") -- so the
 * local product can overlap the all-gather of the remote rows.
 */
int appnp_graph_create_rows(const int32_t* indptr, const int32_t* indices, const float* vals,
                            int64_t n, int64_t nnz, int mode, int64_t row_lo, int64_t row_hi,
                            int split_local, void* stream, appnp_graph** out);

void appnp_graph_destroy(appnp_graph* g);

/* n (global nodes), rows held [row_lo,row_hi), nnz of the held A_hat rows, symmetric flag
 * (1 if A's pattern and weights are symmetric, so A_hat^T == A_hat for 'sym'). */
int appnp_graph_info(const appnp_graph* g, int64_t* n, int64_t* row_lo, int64_t* row_hi,
                     int64_t* nnz_hat, int* mode, int* symmetric);

/* Read-only device views of the held A_hat CSR (row_ptr is local: row_ptr[0] == 0). */
int appnp_graph_csr(const appnp_graph* g, const int32_t** row_ptr, const int32_t** col,
                    const float** val);

/* Stream-ordered copy of the held A_hat CSR and of dinv into caller-owned device buffers
 * (row_ptr[rows+1], col[nnz_hat], val[nnz_hat], dinv[n]); any pointer may be NULL. */
int appnp_graph_copy_csr(const appnp_graph* g, int32_t* row_ptr, int32_t* col, float* val,
                         double* dinv, void* stream);

/* Device bytes of the source-blocked copy (APPNP_GRAPH_SOURCE_BLOCKS); 0 if not built. */
int appnp_graph_source_blocks(const appnp_graph* g, int64_t* bytes);

/* Device view of the fp64 inverse-degree vector (1/sqrt(D) for sym, 1/D for rw), length n. */
int appnp_graph_dinv(const appnp_graph* g, const double** dinv);

/* Bytes of workspace appnp_propagate / appnp_propagate_bwd need for this shape.  The
 * workspace holds the ping-pong iterates with its own line-aligned leading dimension, or the
 * two buffers of the split layout ([n, fs] + [n, width of the source-blocked copy]), whichever
 * is larger (`ld` is accepted for ABI stability and ignored). */
size_t appnp_workspace_bytes(const appnp_graph* g, int64_t f, int64_t ld, int dtype);

/* The column split appnp_propagate uses for this shape when H and Z are 16-B aligned with
 * leading dimensions that are multiples of 4 floats (K >= 2): columns [0, *fs) gather whole cache
 * lines and [*fs, F) run the persistent L2-blocked remainder pass.  fp32 rows of F = 32q + r
 * features take it on a graph built with a source-blocked copy, above 2^16 nodes and without
 * gather locality: r <= 4 on an APPNP_GRAPH_SOURCE_BLOCKS copy, r <= 8 on an APPNP_GRAPH_SB_W8
 * copy (wider remainders beside a main part keep whole rows, and so does every F > 32 on an
 * APPNP_GRAPH_SB_W16 copy).  *fs = 0 when rows are
 * gathered whole, and also for narrow rows, which run wholly in the pass (see below).
 * Informational: appnp_propagate decides by itself, on the same rule. */
int appnp_propagate_split_point(const appnp_graph* g, int64_t f, int dtype, int64_t* fs);

/* The remainder columns of that split: *r = F - fs columns run the L2-blocked pass -- 1-4 on an
 * APPNP_GRAPH_SOURCE_BLOCKS copy, up to 8 on a W8 copy -- and narrow rows F <= 4 / 8 / 16
 * (the copy's width) run wholly in the pass, *r = F with *fs = 0.  *r = 0 when rows are
 * gathered whole. */
int appnp_propagate_remainder_cols(const appnp_graph* g, int64_t f, int dtype, int64_t* r);

/* The source-blocked copy as built: *width remainder columns per row (4, 8, 16; 0 = not built),
 * *entries regrouped entries including padding, *value_free = 1 when entries carry no values
 * (unit graph: A_hat_ij = dl_i dr_j), *row_passes row-group passes per launch, and *launches the
 * remainder-pass launches enqueued on this graph so far (which path a propagation took). */
int appnp_graph_source_block_layout(const appnp_graph* g, int* width, int64_t* entries,
                                    int* value_free, int* row_passes, int64_t* launches);

/*
 * Z = APPNP_K(H):  Z_0 = H;  Z_{k+1} = (1-alpha) (M_k o A_hat) Z_k + alpha H,  k < K.
 *   H, Z: n x f, leading dims ld_h / ld_z, `dtype` storage; must not alias.
 *   p_drop in [0,1): edge dropout; M_k keeps edge (i,j) at step k iff the 24-bit counter
 *   hash of (seed, k, i, j) >= p_drop * 2^24, and scales kept edges by 1/(1-p_drop).
 *   p_drop = 0 is eval mode (the reference's semantics).
 *   ws: appnp_workspace_bytes() bytes (may be NULL when that is 0).
 * One fused kernel launch per iteration.  With split rows (appnp_propagate_remainder_cols >
 * 0) an iteration is that launch on the first fs columns (none for narrow rows) plus ONE
 * persistent launch of the L2-blocked remainder pass over every source block, and H is first
 * copied into the workspace's split layout.  All launches are stream-ordered on `stream`;
 * nothing is allocated or synchronised.  Requires a full (non-partitioned) graph.
 */
int appnp_propagate(const appnp_graph* g, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
                    int64_t f, int dtype, int K, float alpha, float p_drop, uint64_t seed,
                    void* ws, size_t ws_bytes, void* stream);

/*
 * dH = J^T dZ for the map H -> Z of appnp_propagate with the same (K, alpha, p_drop, seed).
 * Uses A_hat^T: A_hat itself for 'sym' on an undirected graph, otherwise the transpose built
 * at creation with APPNP_GRAPH_TRANSPOSE; APPNP_ENOTSUP if neither is available.  On a
 * self-adjoint A_hat it uses the same column split as appnp_propagate.
 */
int appnp_propagate_bwd(const appnp_graph* g, const void* dZ, int64_t ld_dz, void* dH,
                        int64_t ld_dh, int64_t f, int dtype, int K, float alpha, float p_drop,
                        uint64_t seed, void* ws, size_t ws_bytes, void* stream);

/*
 * Exact PPNP: Z = Pi H with Pi = alpha (I - (1-alpha) A_hat)^-1 (helpers.py:68-71 compute_ppr,
 * model.py:63), to a stated tolerance, without the dense inverse.  The fixed point of
 * Z = (1-alpha) A_hat Z + alpha H is reached by Chebyshev semi-iteration instead of the plain
 * series of appnp_propagate.  On an undirected graph ('sym' or 'rw') the spectrum of
 * (1-alpha) A_hat is real and lies in [-rho, rho], rho = 1 - alpha, so
 *
 *   Z_0 = H,   Z_{k+1} = w_{k+1} ((1-alpha) A_hat Z_k + alpha H) + (1 - w_{k+1}) Z_{k-1},
 *   w_1 = 1,   w_2 = 1 / (1 - rho^2 / 2),   w_{k+1} = 1 / (1 - rho^2 w_k / 4)
 *
 * shrinks the error by sigma = rho / (1 + sqrt(1 - rho^2)) per step (0.627 at alpha = 0.1,
 * against 0.9 for the plain series): after m steps it is at most 2 sigma^m / (1 + sigma^2m) of
 * the initial one.
 *
 * appnp_solve_iterations  *iters = the smallest m >= 1 with 2 sigma^m / (1 + sigma^2m) <= tol
 *                         (alpha = 0.1: tol 1e-5 / 1e-6 / 1e-7 -> 27 / 32 / 36).  Host only.
 *                         APPNP_EINVAL unless 0 < alpha <= 1 and 0 < tol < 1; APPNP_ERANGE when
 *                         alpha is so small that no count below 2^20 reaches tol.
 * appnp_solve_weights     omega[0 .. iters) = w_1 .. w_iters in fp64.  Host only.
 * appnp_solve             `iters` steps from Z_0 = H, the last one into Z: one launch of the
 *                         fused SpMM kernel per step (timed as APPNP_KT_STEP), whose epilogue
 *                         reads one extra row, Z_{k-1}.  The count is fixed a priori, so no
 *                         residual is read back: stream-ordered, no allocation, graph-capturable,
 *                         like appnp_propagate.  ws: appnp_workspace_bytes() bytes.
 * appnp_solve_bwd         dH = Pi^T dZ: the same solve on A_hat^T (A_hat itself for 'sym', the
 *                         transpose built with APPNP_GRAPH_TRANSPOSE for 'rw'; APPNP_ENOTSUP
 *                         without it).  This is the gradient of the CONVERGED operator H -> Pi H,
 *                         exact to the same tolerance -- not the adjoint of a loop truncated at
 *                         `iters` steps.
 * Limits: a full graph; H != Z; fp32 only (APPNP_ENOTSUP for bf16); an undirected graph only
 * (APPNP_ENOTSUP when the graph's symmetric flag is 0: a directed A_hat has a complex spectrum
 * and the recurrence may diverge); no dropout (a mask that changes per step has no fixed point).
 * Rows are always gathered whole: the source-blocked remainder pass is not used, also on a graph
 * that has the copy, and appnp_graph_source_block_layout's launch count does not move.
 * Arguments are validated before any device call.
 */
int appnp_solve_iterations(float alpha, float tol, int* iters);
int appnp_solve_weights(float alpha, int iters, double* omega);
int appnp_solve(const appnp_graph* g, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
                int64_t f, int dtype, int iters, float alpha, void* ws, size_t ws_bytes,
                void* stream);
int appnp_solve_bwd(const appnp_graph* g, const void* dZ, int64_t ld_dz, void* dH, int64_t ld_dh,
                    int64_t f, int dtype, int iters, float alpha, void* ws, size_t ws_bytes,
                    void* stream);

/*
 * Polynomial propagation (GPR-GNN; the generalisation of the APPNP series):
 *
 *   Z = sum_{k=0..K} gamma_k A_hat^k H
 *
 * gamma_k = alpha (1-alpha)^k (k < K), gamma_K = (1-alpha)^K is appnp_propagate(K, alpha);
 * gamma_k = e^-t t^k / k! is heat-kernel diffusion; a trained gamma is GPR-GNN, negative
 * (high-pass) coefficients included.  coef: K + 1 fp32 values in DEVICE memory, read by the
 * kernels only, so a trainable gamma never crosses to the host and a captured call follows a
 * refill of it.
 *
 * appnp_poly      T_0 = H, T_k = A_hat T_{k-1}, Z = sum gamma_k T_k: K launches of the fused SpMM
 *                 kernel (APPNP_KT_STEP; the first also forms gamma_0 H, the last stores no T_K);
 *                 K = 0: one row-scale launch (APPNP_KT_COPY), Z = gamma_0 H.
 * appnp_poly_bwd  From <dZ, A_hat^k H> = <(A_hat^T)^k dZ, H>: G_0 = dZ, G_k = A_hat^T G_{k-1},
 *                 dH = sum gamma_k G_k and dcoef[k] = <G_k, H>; no power of A_hat times H is stored
 *                 or recomputed.  One row launch (dH = gamma_0 dZ and the row dots of <dZ, H>), K
 *                 step launches whose epilogue also leaves one fp32 partial of <G_k, H> per (column
 *                 slab, row), and K + 1 reduce launches (APPNP_KT_COPY) of one fixed shape: 1024
 *                 threads, thread t sums partials t, t + 1024, ... in fp64, then a halving tree.
 *                 No floating-point atomics: dH and dcoef are bitwise reproducible.  dcoef: K + 1
 *                 fp32 in device memory, or NULL: then no dot is computed and H may be NULL.
 *                 A_hat^T is A_hat itself for 'sym' on a symmetric graph, else the transpose built
 *                 with APPNP_GRAPH_TRANSPOSE; APPNP_ENOTSUP if neither is available.
 * appnp_poly_workspace_bytes  bytes of `ws` for either call (with_dcoef: appnp_poly_bwd with a
 *                 non-NULL dcoef): up to two [n, f] buffers and the partial dots.  Monotone in f
 *                 and K; 0 for an empty shape or invalid arguments.
 * Both calls are stream-ordered, allocate nothing and never synchronise.
 * Limits: a full graph ('sym' or 'rw', directed graphs included, for the forward); H != Z,
 * dZ != dH, H != dH; 0 <= K <= APPNP_POLY_MAX_K; fp32 only (APPNP_ENOTSUP for bf16); no edge
 * dropout (a mask per step breaks the identity behind dcoef).  Rows are always gathered whole:
 * the source-blocked remainder pass is not used, also on a graph that has the copy, and
 * appnp_graph_source_block_layout's launch count does not move.  Arguments are validated before
 * any device call, in the order of appnp_solve; an empty shape (n = 0 or f = 0) is APPNP_OK.
 */
#define APPNP_POLY_MAX_K 1024
size_t appnp_poly_workspace_bytes(const appnp_graph* g, int64_t f, int K, int with_dcoef);
int appnp_poly(const appnp_graph* g, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
               int64_t f, int dtype, int K, const float* coef, void* ws, size_t ws_bytes,
               void* stream);
int appnp_poly_bwd(const appnp_graph* g, const void* dZ, int64_t ld_dz, const void* H,
                   int64_t ld_h, void* dH, int64_t ld_dh, float* dcoef, int64_t f, int dtype,
                   int K, const float* coef, void* ws, size_t ws_bytes, void* stream);

/*
 * Sparse top-k PPR rows (batch-main.py:113-117, 134-152: the dense `ppr.topk` and the per-batch
 * `model.ppr[idx_batch]` / `(ppr_sub > 0).any(dim=0)`): the k largest entries of every COLUMN of
 * a row-major block, as the rows of a canonical CSR.
 *   X: [n, b] fp32, leading dimension ld_x >= b -- the layout appnp_solve / appnp_propagate
 *      write, Pi[:, idx] for b source nodes.
 *   The candidate of (row r, column c) is v = (X[r, c] * rs) * cs in fp32, in that order, with
 *   rs = row_scale[r] and cs = col_scale[c]; a NULL scale means no multiplication at all ('rw':
 *   Pi[i, :] = D * Pi[:, i] / d_i with row_scale = D, col_scale = 1 / D[idx]).
 *   Per column the k rows with the largest v are kept.  The order is total: equal values go by
 *   the smaller row index, -0 equals +0, a NaN orders below every number (below -inf), and among
 *   NaNs the lower index comes first.
 *   out_idx[c * ld_out + j], out_val[c * ld_out + j], j < k: the kept rows of column c in
 *   ASCENDING row index with their values v -- CSR row c of a b x n matrix with exactly k entries
 *   per row, so its row pointer is k * arange(b + 1) and nothing has to be read back.  Elements
 *   j >= k of an output row are not written (ld_out >= k).
 *   ws: appnp_topk_workspace_bytes(n, b, k) bytes (monotone in n and b; 0 for an empty shape).
 * The reference keeps every entry >= the k-th value (more than k on ties); this keeps exactly k.
 * A chain of launches on `stream` (radix select, 8 bits per pass, on the order-preserving integer
 * image of v; then count, scan and emit passes; X is read 6 times): stream-ordered, no allocation,
 * no host synchronisation, graph-capturable, integer atomics only and therefore bitwise
 * reproducible.  The per-launch timer records its launches as APPNP_KT_COPY.
 * APPNP_EINVAL, before any device call: n < 0, b < 0, ld_x < b, k < 1, ld_out < k, n > INT32_MAX;
 * then APPNP_OK when n * b == 0; then APPNP_EINVAL for k > n, a NULL X / out_idx / out_val / ws,
 * or ws_bytes too small.  APPNP_ERANGE when n * b exceeds what one launch can cover (2^39).
 */
size_t appnp_topk_workspace_bytes(int64_t n, int64_t b, int k);
int appnp_topk_columns(const float* X, int64_t ld_x, int64_t n, int64_t b, int k,
                       const float* row_scale, const float* col_scale, int32_t* out_idx,
                       float* out_val, int64_t ld_out, void* ws, size_t ws_bytes, void* stream);

/*
 * PPR columns by local forward push (Andersen-Chung-Lang): X = Pi[:, sources], the block
 * appnp_topk_columns reads, at a cost per source that follows its residual (about 1 / eps and the
 * local neighbourhood) instead of n.  A third way to the columns, beside the K-step series
 * (appnp_propagate) and the solver (appnp_solve) of one-hot columns.
 *
 * Per source s, with T = (1 - alpha) A_hat: an estimate p and a residual r, int64 fixed point in
 * units of 2^-44; p = 0, r = e_s (2^44 at s).  A round is synchronous.  Its frontier is
 * F = { j : r_j >= thr_j }, thr_j = max(1, ceil(eps w_j 2^44)) in fp64, w_j = 1 / dinv_j
 * (= sqrt(d_j)) for 'sym' and 1 for 'rw'.  Every i in F is taken (t = r_i, r_i = 0) before
 * anything is added; then p_i += (int64)((double)t * (double)alpha) and, for every entry (j, i)
 * of column i of A_hat, r_j += (int64)(((double)t * (double)val) * (double)(1.0f - alpha)), both
 * conversions truncating, alpha and val the fp32 values.  It stops when F is empty or after
 * max_rounds rounds.  X[j, c] = (float)((double)p_j 2^-44).  All sums are integer sums and a
 * round is a pure function of the state before it: the result is bitwise reproducible and does
 * not depend on scheduling.  With F empty, |Pi[j, s] - X[j, c]| < eps w_j (eps sqrt(d_j) for sym,
 * eps for rw).  A_hat >= 0 is assumed (unweighted graphs, non-negative weights): a graph that
 * violates it can give wrong numbers, never an out-of-range access.
 *
 *   sources: b node indices (device memory); duplicates are independent columns; an index
 *      outside [0, n) gives an all-zero column with left = -1.
 *   X: [n, b] fp32, ld_x >= b; every element of X[:, :b] is written, padding columns are not.
 *   rounds[c]: rounds run for column c; left[c]: frontier size at exit, 0 = the bound holds.
 *      Each may be NULL.
 *   ws: appnp_push_workspace_bytes(n, b) bytes (monotone in n and b; 0 for an empty shape), 16-byte
 *      aligned: per source r, p and the takes of a round as int64 [n] and two frontier lists of
 *      capacity n as int32, plus the n thresholds.  The call clears r and p on the stream itself.
 * Column i of A_hat is row i of A_hat^T: 'sym' walks the stored CSR, 'rw' the transpose built with
 * APPNP_GRAPH_TRANSPOSE.  One workgroup per source with the whole round loop inside one launch
 * (timed as APPNP_KT_PUSH; the clear, the thresholds and the final p -> X launch as
 * APPNP_KT_COPY): workgroup barriers only, no workgroup waits for another, 64-bit integer atomics
 * only.  Stream-ordered, no allocation, no host synchronisation, graph-capturable.
 * APPNP_EINVAL, before any device call: a NULL g, b < 0, ld_x < b, alpha outside (0, 1], eps
 * outside (0, 1), max_rounds < 1; then APPNP_OK when b == 0 or n == 0; then APPNP_EINVAL for a
 * NULL sources / X / ws or ws_bytes too small.  APPNP_ENOTSUP: a row-partitioned graph, a graph
 * whose symmetric flag is 0 (as appnp_solve), 'rw' without the transpose.  fp32 only.
 */
size_t appnp_push_workspace_bytes(int64_t n, int64_t b);
int appnp_push_columns(const appnp_graph* g, const int64_t* sources, int64_t b, float alpha,
                       float eps, int max_rounds, float* X, int64_t ld_x, int32_t* rounds,
                       int32_t* left, void* ws, size_t ws_bytes, void* stream);

/*
 * Sparse top-k PPR rows straight from the forward push: what appnp_push_columns followed by
 * appnp_topk_columns gives for the same arguments -- the same out_idx (ascending, exactly k per
 * source), the same bits in out_val, the same rounds and left -- without the dense n x b block.
 * The cost per source follows the push alone (about 1 / eps and the local neighbourhood), from
 * the push to the CSR row, and the workspace depends on `slots`, not on b: one call can take any
 * number of sources, all n of them included.
 *
 * The push is appnp_push_columns' (same fixed point, rounds and thresholds).  The candidate of
 * (node j, source c) is v = (X * row_scale[j]) * col_scale[c] with X = (float)((double)p_j 2^-44),
 * two separately rounded fp32 products, a NULL scale meaning no multiplication; the order is
 * appnp_topk_columns' (larger v first, equal v to the smaller j), taken on v, not on p.  Only the
 * nodes the push took can have p > 0.  A source with fewer than k positive candidates is filled
 * with +0.0 at the smallest indices that hold none, as the chain does; an index outside [0, n)
 * gives the indices 0 .. k-1 with +0.0 and left = -1.  The identity with the chain holds for
 * scales that are finite and > 0 (the degrees and inverse degrees of 'rw'); with other scales
 * the chain's candidates of untouched nodes are no longer +0.0 and the result is unspecified.
 *
 *   k: 1 .. min(n, APPNP_PUSH_TOPK_MAX_K); out_idx / out_val: [b, k], ld_out >= k, elements
 *      j >= k of a row are not written.
 *   slots: workgroups (of 1024 threads) launched; workgroup w runs the sources w, w + slots, ...
 *      in order on its own slice of the workspace and leaves it clean for the next one, at the
 *      cost of one more walk over the rows of the nodes it took.  min(slots, b) are used.
 *   ws: appnp_push_topk_workspace_bytes(n, slots) bytes (monotone in n and slots, 0 for an empty
 *      shape), 16-byte aligned: per slot r, p and the takes as int64 [n] and three lists of
 *      capacity n as int32 (36 n bytes), plus the n thresholds.
 * Launches on `stream`: one clear of the slots' r and p and the thresholds ('sym') as
 * APPNP_KT_COPY, then ONE launch with the push, the selection (a workgroup-local radix select on
 * the 64-bit keys order_key(v) << 32 | ~j) and the clean-up of every source, as APPNP_KT_PUSH.
 * No workgroup waits for another; integer atomics only, so two runs give the same bits.
 * Stream-ordered, no allocation, no host synchronisation, no read-back, graph-capturable.
 * APPNP_EINVAL, before any device call: a NULL g, b < 0, k < 1, ld_out < k, max_rounds < 1,
 * slots < 1, alpha outside (0, 1], eps outside (0, 1); then APPNP_OK when b == 0 or n == 0; then
 * APPNP_EINVAL for k > n, a NULL sources / out_idx / out_val / ws or ws_bytes too small.
 * APPNP_ENOTSUP: a row-partitioned graph, a graph whose symmetric flag is 0, 'rw' without the
 * transpose, k > APPNP_PUSH_TOPK_MAX_K.  fp32 only.
 */
#define APPNP_PUSH_TOPK_MAX_K 1024
size_t appnp_push_topk_workspace_bytes(int64_t n, int slots);
int appnp_push_topk(const appnp_graph* g, const int64_t* sources, int64_t b, float alpha,
                    float eps, int max_rounds, int k, const float* row_scale,
                    const float* col_scale, int32_t* out_idx, float* out_val, int64_t ld_out,
                    int32_t* rounds, int32_t* left, int slots, void* ws, size_t ws_bytes,
                    void* stream);

/*
 * The per-minibatch slice of a sparse PPR matrix (batch-main.py:140-142: `ppr_sub = ppr[idx]`,
 * `sel = (ppr_sub > 0).any(dim=0)`, `ppr_sub[:, sel]`), with the transpose of the sub-matrix: two
 * calls with ONE read-back between them, the 24 bytes of `counts`, from which the caller sizes the
 * outputs of the second.
 *   P: a CSR [rows, cols], int32 indptr / indices, fp32 vals.  indices / vals may be NULL for a
 *      matrix without entries: every row is then taken as empty.
 *   idx: b row indices (int64, device memory), in any order, duplicates allowed.  Taken row p is
 *      P[idx[p]].  An index outside [0, rows) contributes an empty row and is counted in
 *      counts[2]; the kernels never read outside indptr.
 *   Column j is SELECTED iff some taken entry (p, j) has val > 0: a stored 0.0, -0.0, negative
 *      value or NaN does not select its column (nor does an entry whose column lies outside
 *      [0, cols), which is dropped).  sel: the selected columns, ascending, int64 [n_sel].
 *   An entry of a taken row is KEPT iff its column is selected, whatever its value.  Kept entries
 *      keep their order within the row; their column becomes its rank in sel.
 *   appnp_csr_batch_count writes
 *      out_indptr: int32 [b + 1], the row pointer of the [b, n_sel] result;
 *      counts: int64 [3] = kept entries (nnz_out), n_sel, indices outside [0, rows);
 *   and leaves its state (the bitmap of selected columns and the rank of each of its words) in
 *   the first appnp_csr_batch_workspace_bytes(cols, b, 0) bytes of ws.
 *   appnp_csr_batch_emit, after it on the same stream, with nnz_out = counts[0] and
 *   n_sel = counts[1] and the out_indptr count wrote, reads that state and writes
 *      out_indices int32 [nnz_out], out_vals fp32 [nnz_out]: the CSR [b, n_sel];
 *      sel int64 [n_sel];
 *      t_indptr int32 [n_sel + 1], t_indices int32 [nnz_out], t_vals fp32 [nnz_out]: the
 *      canonical CSR [n_sel, b] of its transpose, the entries of a row ascending by batch
 *      position p (equal p: in their order within row p) -- exactly what appnp_csr_transpose
 *      returns for the sub-matrix, bit for bit.
 *   Sizes other than those count reported give unspecified values, never an access outside the
 *   buffers as sized by the arguments.  Outputs of size 0 may be NULL.
 *   ws: 8-byte aligned; count needs appnp_csr_batch_workspace_bytes(cols, b, 0) bytes, emit
 *      appnp_csr_batch_workspace_bytes(cols, b, nnz_out).  The size is monotone in each argument
 *      and 0 for an empty shape (cols <= 0, b <= 0) or a negative nnz_cap.  A caller that knows a
 *      bound on the kept entries before the read-back passes one workspace to both calls; one that
 *      does not may run count on a workspace of the smaller size and give emit a larger one that
 *      starts with a copy of it.  Beyond the bitmap (cols bits) and its word ranks (cols / 32
 *      words) nothing in it grows with cols: b words, and 8 nnz_cap + 4 min(cols, nnz_cap) bytes.
 * Launches on `stream`: count is a clear and three kernels (mark the bitmap with atomicOr, for
 * cols <= APPNP_CSR_BATCH_LDS_COLS gathered in LDS per workgroup before it is merged; count each
 * taken row; one workgroup that scans the bitmap's popcounts and the row counts,
 * APPNP_CSR_BATCH_SCAN_PASS items per pass); emit is five (sel; a stable in-row compaction;
 * t_indptr from per-column counts; a scatter of the kept entries to their column's segment through
 * an atomic cursor; a sort of each segment by the entry's position in out_indices, which is unique,
 * so the result does not depend on the order the atomics took).  Work per batch follows the taken
 * entries plus cols / 32 words.  No workgroup waits for another; integer atomics only, so two runs
 * give the same bits.  Both calls are stream-ordered and make no allocation and no host
 * synchronisation.  The per-launch timer records their launches as APPNP_KT_COPY.
 * APPNP_EINVAL, before any device call: rows, cols or b negative, cols or b > INT32_MAX; for emit
 * also nnz_out or n_sel negative, nnz_out > INT32_MAX, n_sel > cols, n_sel > nnz_out (every
 * selected column holds a kept entry).  Then APPNP_OK, with nothing written, when b == 0 or
 * cols == 0.  Then APPNP_EINVAL for a NULL indptr / idx / out_indptr / ws, a NULL counts (count) or
 * t_indptr (emit), a NULL array of nnz_out > 0 or n_sel > 0 elements (emit), a workspace that is
 * too small or not 8-byte aligned.
 */
#define APPNP_CSR_BATCH_SCAN_PASS 4096
#define APPNP_CSR_BATCH_LDS_COLS 131072
size_t appnp_csr_batch_workspace_bytes(int64_t cols, int64_t b, int64_t nnz_cap);
int appnp_csr_batch_count(const int32_t* indptr, const int32_t* indices, const float* vals,
                          int64_t rows, int64_t cols, const int64_t* idx, int64_t b,
                          int32_t* out_indptr, int64_t* counts, void* ws, size_t ws_bytes,
                          void* stream);
int appnp_csr_batch_emit(const int32_t* indptr, const int32_t* indices, const float* vals,
                         int64_t rows, int64_t cols, const int64_t* idx, int64_t b,
                         const int32_t* out_indptr, int64_t nnz_out, int64_t n_sel,
                         int32_t* out_indices, float* out_vals, int64_t* sel, int32_t* t_indptr,
                         int32_t* t_indices, float* t_vals, void* ws, size_t ws_bytes,
                         void* stream);

/*
 * Whole rows of a device CSR (`M[idx]`: the rows X[sel] of a sparse attribute matrix, the rows
 * ppr[idx_stop] of a sparse PPR matrix), optionally with the transpose of the slice: two calls
 * with ONE read-back between them, the 16 bytes of `counts`, from which the caller sizes the
 * outputs of the second.
 *   M: a CSR [rows, cols], int32 indptr / indices, fp32 vals.  indices / vals may be NULL for a
 *      matrix without entries: every row is then taken as empty.
 *   idx: b row indices (int64, device memory), in any order, duplicates allowed.  Taken row p is
 *      M[idx[p]], copied whole: its entries keep their order, columns are NOT relabelled, values
 *      are copied bit for bit.  An index outside [0, rows) contributes an empty row and is counted
 *      in counts[1]; the kernels never read outside indptr.
 *   appnp_csr_rows_count writes
 *      out_indptr: int32 [b + 1], the row pointer of the [b, cols] result;
 *      counts: int64 [2] = entries of the result (nnz_out), indices outside [0, rows);
 *   from indptr alone (O(b) work), in ONE single-workgroup launch that folds the row lengths,
 *   their scan (APPNP_CSR_BATCH_SCAN_PASS items per pass) and the out-of-range count: it needs no
 *   workspace and nothing is cleared before it.
 *   appnp_csr_rows_emit, after it on the same stream, with nnz_out = counts[0] and the out_indptr
 *   count wrote, writes
 *      out_indices int32 [nnz_out], out_vals fp32 [nnz_out]: the CSR [b, cols];
 *   and, when t_indptr != NULL,
 *      t_indptr int32 [cols + 1], t_indices int32 [nnz_out], t_vals fp32 [nnz_out]: the canonical
 *      CSR [cols, b] of its transpose, the entries of a row ascending by batch position p (equal
 *      p: in their order within row p) -- exactly what appnp_csr_transpose returns for the slice,
 *      bit for bit.
 *   With t_indptr == NULL only the copy runs (one launch; t_indices, t_vals and ws are not used):
 *   the route for a slice that is never differentiated.
 *   An entry whose column lies outside [0, cols) is copied as it is and left out of the transpose;
 *   the values of such a malformed matrix, and those for sizes other than count reported, are
 *   unspecified, but there is never an access outside the buffers as sized by the arguments.
 *   Outputs of size 0 may be NULL.
 *   ws: only for the transpose of a slice with entries (t_indptr != NULL, nnz_out > 0, cols > 0):
 *      4-byte aligned, appnp_csr_rows_workspace_bytes(cols, nnz_out) bytes: cols cursors and
 *      2 nnz_cap words for the (entry, row) pairs, rounded up to 256 bytes.  The size is monotone
 *      in each argument and 0 for an empty shape (cols <= 0 or nnz_cap <= 0).
 * Launches on `stream`: count is one; emit is one without the transpose, and with it five: a clear
 * of t_indptr (a kernel, not a memset node), the wave-per-row copy that also counts each column
 * with integer atomics, and the t_indptr scan, scatter and segment sort of appnp_csr_batch_emit
 * (the same kernels, over all cols columns).  No workgroup waits for another; integer atomics
 * only, so two runs give the same bits.  Both calls are stream-ordered and make no allocation and
 * no host synchronisation.  The per-launch timer records their launches as APPNP_KT_COPY.
 * APPNP_EINVAL, before any device call: rows, cols or b negative, cols or b > INT32_MAX; for emit
 * also nnz_out negative or > INT32_MAX.  Then APPNP_OK, with nothing written, when b == 0.  Then
 * APPNP_EINVAL for a NULL indptr / idx / out_indptr, a NULL counts (count), a NULL array of
 * nnz_out > 0 elements (emit; t_indices / t_vals only with t_indptr), and, where the workspace is
 * used, one that is NULL, too small or misaligned.
 */
size_t appnp_csr_rows_workspace_bytes(int64_t cols, int64_t nnz_cap);
int appnp_csr_rows_count(const int32_t* indptr, const int32_t* indices, const float* vals,
                         int64_t rows, int64_t cols, const int64_t* idx, int64_t b,
                         int32_t* out_indptr, int64_t* counts, void* stream);
int appnp_csr_rows_emit(const int32_t* indptr, const int32_t* indices, const float* vals,
                        int64_t rows, int64_t cols, const int64_t* idx, int64_t b,
                        const int32_t* out_indptr, int64_t nnz_out, int32_t* out_indices,
                        float* out_vals, int32_t* t_indptr, int32_t* t_indices, float* t_vals,
                        void* ws, size_t ws_bytes, void* stream);

/*
 * One iteration on the held rows:  Zout[i-row_lo] = (1-alpha) sum_j (M_k o A_hat)_ij Zin[j]
 *                                                   + alpha H[i-row_lo],  i in [row_lo,row_hi)
 *   Zin: all n rows (global row index), Zout/H: the held rows only.
 *   part selects which stored CSR is applied:
 *     APPNP_PART_ALL     the held rows' full CSR (epilogue as above)
 *     APPNP_PART_LOCAL   local-column CSR only:  P[i] = (1-alpha) sum_local ...   (P = Zout, fp32)
 *     APPNP_PART_REMOTE  remote-column CSR, finishing: Zout = (1-alpha) sum_remote + P + alpha H
 *                        (P passed as `partial`, fp32, ld = ld_partial)
 */
enum appnp_part { APPNP_PART_ALL = 0, APPNP_PART_LOCAL = 1, APPNP_PART_REMOTE = 2 };

int appnp_step(const appnp_graph* g, int part, const void* Zin, int64_t ld_in, const void* H,
               int64_t ld_h, void* Zout, int64_t ld_out, const float* partial,
               int64_t ld_partial, int64_t f, int dtype, int k, float alpha, float p_drop,
               uint64_t seed, void* stream);

/*
 * Split rows on the held rows of a row-partitioned graph (appnp_graph_create_rows with a
 * source-blocked copy, APPNP_GRAPH_SOURCE_BLOCKS / _SB_W8 / _SB_W16; fp32; the split rule of
 * appnp_propagate_remainder_cols).  The iterate is kept as two FULL-HEIGHT parts (every rank's
 * rows, global row index): main [rows_total, fs] (fs = F - r columns, whole cache lines per
 * gathered row) and rem [rows_total, rem_width] (the r remainder columns, zero padded; on a unit
 * graph scaled by the column scale of A_hat, which only these functions read and write).  Each
 * rank writes its held rows of both parts; an exchange (all-gather) fills the others.  All
 * buffers 16-B aligned, leading dimensions multiples of 4 floats.
 *
 * appnp_split_layout  *fs and *rem_width of that layout for F; APPNP_ENOTSUP when F does not
 *                     split on this graph (then use appnp_step).
 * appnp_split_copy    the held rows of H (ld_h) into rows [row_lo, row_hi) of main and rem: the
 *                     Z_0 parts.  main may be NULL when fs = 0.
 * appnp_step_split    one iteration of the held rows from all rows of zin_main / zin_rem:
 *                     into rows [row_lo, row_hi) of zout_main / zout_rem, or, when Z != NULL,
 *                     into the held rows of Z (ld_z, all F columns: the last iteration).  part
 *                     as for appnp_step, on the main columns: ALL (then the remainder pass),
 *                     LOCAL (local-column product of the main part into the fp32 `partial`
 *                     [held rows, fs], ld_partial; zin_rem is not read, so it may still be in
 *                     flight), REMOTE (remote columns + partial + alpha H, then the remainder
 *                     pass).  LOCAL / REMOTE need split_local.  Stream-ordered, no allocation.
 * the north_star's row partition gathers q lines per nonzero for F = 32q + r
 * instead of q + 1, as the single-GPU appnp_propagate does.
 */
int appnp_split_layout(const appnp_graph* g, int64_t f, int64_t* fs, int64_t* rem_width);
int appnp_split_copy(const appnp_graph* g, const float* H, int64_t ld_h, int64_t f, float* main,
                     float* rem, void* stream);
int appnp_step_split(const appnp_graph* g, int part, const float* zin_main, const float* zin_rem,
                     const float* H, int64_t ld_h, float* zout_main, float* zout_rem, float* Z,
                     int64_t ld_z, float* partial, int64_t ld_partial, int64_t f, int k,
                     float alpha, float p_drop, uint64_t seed, void* stream);

/*
 * Pipelined row steps.  A row rank's product split by
 * SOURCE SHARD: with the held rows' entries grouped by the shard of their column (rank s of P
 * holds rows [s S, (s+1) S)), the product over the shards that have already arrived can run while
 * the others are still in flight, one launch per group of shards, so only the last group's share
 * of the compute is left after the exchange ends.
 *
 * appnp_graph_shard_offsets  build the held rows' shard offsets (nshards = P, shard_rows = S,
 *                            P S >= n; (P + 1) x rows int32 of device memory).  Allocates and
 *                            synchronises; idempotent for the same P and S.
 * appnp_step_shards          one iteration's product over the entries of the held rows whose
 *                            column lies in shards [s_lo, s_hi) (fp32):
 *                              APPNP_SHARDS_FIRST  partial  = (1-alpha) sum
 *                              APPNP_SHARDS_ACC    partial += (1-alpha) sum
 *                              APPNP_SHARDS_LAST   Zout     = (1-alpha) sum + partial + alpha H
 *                              APPNP_SHARDS_ONLY   Zout     = (1-alpha) sum + alpha H
 *                            Zin: all n rows (only the range's rows are read); partial [held rows,
 *                            f] fp32.  Summing every shard once, in any grouping, gives the
 *                            appnp_step result up to fp32 summation order.
 * appnp_step_split_shards    the same on the split layout of appnp_step_split: the main columns
 *                            take the shard range and mode; LAST / ONLY then run the remainder
 *                            pass (which needs every row of zin_rem) and write zout_* or Z.
 * Stream-ordered, no allocation; the dropout hash is the same as appnp_step's.
 */
enum appnp_shard_mode {
  APPNP_SHARDS_FIRST = 0,
  APPNP_SHARDS_ACC = 1,
  APPNP_SHARDS_LAST = 2,
  APPNP_SHARDS_ONLY = 3
};
int appnp_graph_shard_offsets(appnp_graph* g, int nshards, int64_t shard_rows, void* stream);
int appnp_step_shards(const appnp_graph* g, int s_lo, int s_hi, int mode, const float* Zin,
                      int64_t ld_in, const float* H, int64_t ld_h, float* Zout, int64_t ld_out,
                      float* partial, int64_t ld_partial, int64_t f, int k, float alpha,
                      float p_drop, uint64_t seed, void* stream);
int appnp_step_split_shards(const appnp_graph* g, int s_lo, int s_hi, int mode,
                            const float* zin_main, const float* zin_rem, const float* H,
                            int64_t ld_h, float* zout_main, float* zout_rem, float* Z,
                            int64_t ld_z, float* partial, int64_t ld_partial, int64_t f, int k,
                            float alpha, float p_drop, uint64_t seed, void* stream);

/*
 * A captured propagation plan: the K launches of appnp_propagate for FIXED buffers (H, Z, ws)
 * and parameters, recorded once into a hipGraph and replayed by appnp_plan_launch on any
 * stream with a single graph launch.  For small, launch-bound graphs and serving loops that
 * refill H in place.  Creating a plan captures on an internal stream (no kernels run).
 */
typedef struct appnp_plan appnp_plan;
int appnp_plan_create(const appnp_graph* g, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
                      int64_t f, int dtype, int K, float alpha, float p_drop, uint64_t seed,
                      void* ws, size_t ws_bytes, appnp_plan** out);
/* The same for appnp_solve: its `iters` launches (a linear chain) captured into a plan. */
int appnp_plan_create_solve(const appnp_graph* g, const void* H, int64_t ld_h, void* Z,
                            int64_t ld_z, int64_t f, int dtype, int iters, float alpha, void* ws,
                            size_t ws_bytes, appnp_plan** out);
int appnp_plan_launch(const appnp_plan* p, void* stream);
void appnp_plan_destroy(appnp_plan* p);

/*
 * Row-partitioned multi-GPU propagation: SURVEY.md 8(b)'s appnp_dist_create, the loop of
 * ppnp_amd/dist.py PartitionedAPPNP.run for a pure row layout, and the replacement of the
 * reference's single-device product model.py:63 for graphs that outgrow one GPU.
 *
 * Rank r of P holds rows [r S, min(n, (r+1) S)) of A_hat, S = ceil(n / P).  After every
 * iteration but the last, the ranks exchange their new row shards through a caller-supplied
 * all-gather, so the library owns no communicator.  With overlap, each iteration first
 * applies the local-column part of the rows on `stream`, while the previous exchange still
 * runs on an internal stream, then waits for it and finishes with the remote columns.
 */
typedef struct appnp_dist appnp_dist;

/*
 * In-place all-gather of equal row shards.  `buf` is a device buffer of nranks * shard_bytes;
 * this rank's shard sits at rank * shard_bytes and is complete in stream order on `stream`.
 * The function must leave every rank's shard in place in stream order on `stream`. It can
 * enqueue the exchange there, as ncclAllGather(buf + rank * shard_bytes, buf, shard_bytes,
 * ncclChar, comm, stream) does (appnp_allgather_rccl). Or it can synchronise `stream`, exchange
 * and return.  It returns 0 or a negative code, which appnp_dist_propagate passes on.
 */
typedef int (*appnp_allgather_fn)(void* buf, size_t shard_bytes, int rank, int nranks,
                                  void* stream, void* ctx);

/* indptr/indices/vals/n/nnz/mode: the WHOLE graph's A on this device, as appnp_graph_create.
 * `mode` may carry APPNP_GRAPH_SOURCE_BLOCKS / _SB_W8 / _SB_W16: then fp32 propagations whose
 * F splits (appnp_split_layout) with 16-B aligned H / Z run on the split layout (main part
 * gathers whole lines, remainder pass; appnp_step_split).  Every rank must take that path or
 * none: the rule is the same on every rank (its gather-locality measure is taken over the whole
 * A), and since the copy is best-effort, the first fp32 propagation with K >= 2 agrees through
 * one small exchange in the workspace that every rank built it (that call synchronises the
 * stream once).  A rank whose agreement fails after that exchange keeps failing (the handle is
 * poisoned: every later call returns the stored error without exchanging); a failure before it
 * (the flag's memset, or the callback itself) leaves the peers waiting in that exchange, as
 * any collective does when one rank drops out, so the caller must then end its communicator.
 * The decision does not depend on H or Z: a rank whose H or Z is not 16-B aligned (base pointer
 * or leading dimension) stages it through the workspace, so every rank exchanges the same
 * parts.
 * overlap != 0 keeps the held rows as local- and remote-column CSRs (fp32 propagation only).
 * allgather/ctx: the exchange, called by every rank once per exchanged iterate (twice on the
 * split layout: its main part, then its remainder part). */
int appnp_dist_create(const int32_t* indptr, const int32_t* indices, const float* vals,
                      int64_t n, int64_t nnz, int mode, int rank, int nranks, int overlap,
                      appnp_allgather_fn allgather, void* ctx, void* stream, appnp_dist** out);

/* The held rows [row_lo, row_hi), the shard height S, and the graph of those rows. */
int appnp_dist_rows(const appnp_dist* d, int64_t* row_lo, int64_t* row_hi, int64_t* shard);
const appnp_graph* appnp_dist_graph(const appnp_dist* d);

/* Workspace of appnp_dist_propagate: two full-height iterates (P S rows, line-aligned, or the
 * two parts of the split layout) and, with overlap, the fp32 local-column partial of the held
 * rows; the larger of the two layouts when F splits, the split one with room to stage a
 * misaligned H and Z ([S, F rounded up to 4] fp32 each). */
size_t appnp_dist_workspace_bytes(const appnp_dist* d, int64_t f, int dtype);

/*
 * Z = the held rows of APPNP_K(H), given the held rows of H (row_hi - row_lo rows each;
 * leading dimensions ld_h, ld_z; same semantics, dropout hash and results as appnp_propagate
 * on the whole graph).  Collective: every rank calls it with the same f, dtype, K, alpha,
 * p_drop and seed.  Stream-ordered on `stream`; no allocation; the exchange callback runs on
 * the calling thread.
 */
int appnp_dist_propagate(appnp_dist* d, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
                         int64_t f, int dtype, int K, float alpha, float p_drop, uint64_t seed,
                         void* ws, size_t ws_bytes, void* stream);
void appnp_dist_destroy(appnp_dist* d);

/*
 * The pipelined exchange of the row loop.  With overlap and
 * P >= 3 ranks, a broadcast callback makes appnp_dist_propagate send every iterate as P in-place
 * broadcasts, one row shard each (roots 0 .. P-1 in turn, on the engine's exchange stream, each
 * followed by an event), and run the product as appnp_step(_split)_shards launches: FIRST on the
 * rank's own shard, then ACC per group of arrived remote shards (sized 1, 2, 4, ... from the last
 * to arrive, appnp_dist_pipeline_groups), LAST on the last group -- so after the exchange only
 * one shard's share of the product is left instead of every remote shard's.  The split layout's
 * remainder part keeps the all-gather (it is exchanged first).  Collective: every rank sets it.
 * appnp_bcast_fn: in-place broadcast of `bytes` at `buf` from rank `root` to every rank, in stream
 * order on `stream` (ncclBroadcast(buf, buf, bytes, ncclChar, root, comm, stream) for RCCL:
 * appnp_bcast_rccl), or synchronous; returns 0 or a negative code.
 * appnp_dist_set_broadcast builds the held rows' shard offsets (allocates, synchronises `stream`);
 * APPNP_ENOTSUP without overlap or with P < 3 (one remote shard: nothing to pipeline).
 */
typedef int (*appnp_bcast_fn)(void* buf, size_t bytes, int root, int nranks, void* stream,
                              void* ctx);
int appnp_dist_set_broadcast(appnp_dist* d, appnp_bcast_fn fn, void* ctx, void* stream);
/* The groups [lo[i], hi[i]) of remote shards, *n_out of them (0: not pipelined). */
int appnp_dist_pipeline_groups(const appnp_dist* d, int* lo, int* hi, int max, int* n_out);
int appnp_bcast_rccl(void* buf, size_t bytes, int root, int nranks, void* stream, void* ctx);

/* appnp_allgather_fn over RCCL; ctx is the ncclComm_t of the P ranks, rank order = row order.
 * RCCL is resolved at first use (the librccl.so.1 already loaded in the process, e.g.
 * PyTorch's, else the system one; APPNP_RCCL_LIB overrides), so the library does not link it.
 * APPNP_ENOTSUP if it cannot be loaded, APPNP_EDEVICE if the call fails. */
int appnp_allgather_rccl(void* buf, size_t shard_bytes, int rank, int nranks, void* stream,
                         void* ctx);

/*
 * Measurement aid (no counterpart in the reference): gathers `lines` random 128-B lines of the
 * device buffer `table` (table_bytes, 128-B aligned; read only) on `stream`, 8 lanes per line
 * and 64 lines in flight per wave, line indices hashed from `seed`.  The caller times it with
 * events; lines / time is the box's random-line rate, the quantity that bounds the SpMM on a
 * uniform random graph.  bench.py runs it before its timed region
 * (roofline.box_line_rate).  `sink`: one device float, written only if the gathered sum hits a
 * sentinel value.
 */
int appnp_line_rate_probe(const void* table, int64_t table_bytes, int64_t lines, uint64_t seed,
                          float* sink, void* stream);

/*
 * Measurement aid (no counterpart in the reference): the device time of every launch of the
 * calls made between appnp_kernel_timer_begin and appnp_kernel_timer_end on the calling thread.
 * While the timer is on, appnp_propagate, appnp_propagate_bwd, appnp_step, appnp_step_split
 * and appnp_split_copy (and so appnp_dist_propagate) bracket each launch by two timing events on
 * its stream, one right before and one right after it, tagged with its kind; appnp_dist_propagate
 * brackets each exchange call the same way (APPNP_KT_XCHG, on the stream it is enqueued on).  So
 * an interval covers its launch only: a wait for another stream, or host time, before a launch is
 * never counted in it (`stream` of begin is unused).  The events sit between launches that are
 * stream-ordered anyway, so the launches run as they would without them, but a call timed this
 * way is not graph-capturable, and a replayed plan (appnp_plan_launch) records nothing.  end
 * waits for the events and writes, for the first min(n, max) launches, kinds[i] (APPNP_KT_*) and
 * ms[i], NaN if the pair cannot be timed.  *n_out = launches recorded; APPNP_ERANGE if more than
 * max_launches were enqueued (the rest were not timed).  bench.py prints the split of one
 * propagation as roofline.kernel_ms.
 */
enum appnp_kernel_kind {
  APPNP_KT_COPY = 1,   /* H (or dZ) into the split layout, or a plain copy / scale of rows  */
  APPNP_KT_STEP = 2,   /* the fused SpMM + AXPBY kernel (whole rows or the main columns)   */
  APPNP_KT_REM = 3,    /* the persistent L2-blocked remainder pass                          */
  APPNP_KT_LOCAL = 4,  /* appnp_step(_split) PART_LOCAL: the local-column product           */
  APPNP_KT_REMOTE = 5, /* appnp_step(_split) PART_REMOTE: the remote columns + epilogue     */
  APPNP_KT_XCHG = 6,   /* appnp_dist_propagate: one call of the exchange (all-gather)       */
  APPNP_KT_PUSH = 7    /* appnp_push_columns: the forward-push launch (all rounds)          */
};
int appnp_kernel_timer_begin(int max_launches, void* stream);
int appnp_kernel_timer_end(float* ms, int* kinds, int max, int* n_out);

/*
 * Tuning overrides.  A few environment variables (appnp_tuning_names: ';'-separated) reshape
 * kernels for the measurement sweeps of tools/ -- vector width, entries in flight, the split
 * rule, the remainder pass's block size and barriers.  The library reads them only when
 * APPNP_TUNING=1 is set too; otherwise they are ignored and the measured defaults run.
 * appnp_tuning_overrides returns the ones in effect in this process ("NAME=value;..."), "" when
 * none; bench.py prints it as build.overrides.
 */
const char* appnp_tuning_overrides(void);
const char* appnp_tuning_names(void);

#ifdef __cplusplus
}
#endif

#endif /* PPNP_AMD_H */
