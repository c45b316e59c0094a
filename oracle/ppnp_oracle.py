"""CPU oracle for the APPNP propagation path -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may
import this module, and only as the checker / the timed CPU baseline.  The product path
(``ppnp_amd``) never imports it and has no CPU fallback.

It restates, in numpy/scipy (fp64) and torch.sparse (fp32 CPU baseline), the reference
operator that the HIP path replaces:

* ``calc_a_hat``      -- /root/reference/helpers.py:58-66  (A+I, weighted row-sum degree,
                         ``sym``  D^-1/2 (A+I) D^-1/2   or   ``rw``  D^-1 (A+I))
* ``compute_ppr``     -- /root/reference/helpers.py:68-71  (dense alpha (I-(1-alpha)A_hat)^-1)
* ``appnp_propagate`` -- the K-truncated Neumann series of compute_ppr:
                         Z_0 = H, Z_{k+1} = (1-alpha) A_hat Z_k + alpha H
* ``ppnp_forward``    -- /root/reference/model.py:61-67 propagation step ``ppr[idx] @ H``
* ``standardize``     -- /root/reference/ppnp/data/sparsegraph.py:191-222 (+ helpers 300-395)
* ``synth_graph``     -- the seeded uniform generator of SURVEY.md section 8(d)
* ``edge_keep_mask``  -- the counter-hash edge-dropout mask the HIP kernel uses (no reference
                         oracle exists for edge dropout; this pins the
                         device mask bit-for-bit instead)
* ``round_bf16`` / ``step_exact`` / ``close_bf16_step`` / ``envelope`` -- the bf16 storage
                         reference: one step of the kernel must land within half a bf16 spacing
                         of the exact result plus an fp32 accumulation bound, element by element

Parity pin: ``tests/test_oracle.py`` checks every function above against the golden vectors
in ``tests/golden/*.npz``, which ``tests/golden/make_golden.py`` produced by importing the
reference's own ``helpers``/``model``/``SparseGraph`` in the build container.
"""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

# --------------------------------------------------------------------------------------
# Operator construction (helpers.py:58-66)
# --------------------------------------------------------------------------------------


def _merge_self_loops(indptr, indices, data, n):
    """A + I on CSR arrays, scipy-canonical: sorted columns, diagonal merged (a_ii + 1),
    entries whose value is exactly 0 pruned (scipy's csr_binop_csr drops zero results).
    Follows helpers.py:59 ``adj + sp.eye(adj.shape[0])`` (fp32 + fp64 -> fp64)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    same_row = rows[1:] == rows[:-1]
    if not np.any((indices[1:] <= indices[:-1]) & same_row):
        return _merge_self_loops_sorted(indptr, indices, data, rows, n)
    # canonicalise (sum duplicates, sort) exactly as scipy would before the add
    coo = sp.coo_matrix((data, (rows, indices)), shape=(n, n))
    coo.sum_duplicates()
    r = np.concatenate([coo.row.astype(np.int64), np.arange(n, dtype=np.int64)])
    c = np.concatenate([coo.col.astype(np.int64), np.arange(n, dtype=np.int64)])
    v = np.concatenate([coo.data.astype(np.float64), np.ones(n, dtype=np.float64)])
    key = r * n + c
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    uniq, start = np.unique(key, return_index=True)
    vsum = np.add.reduceat(v, start)  # a_ii + 1 where the diagonal existed
    keep = vsum != 0.0
    uniq, vsum = uniq[keep], vsum[keep]
    rr, cc = uniq // n, uniq % n
    out_ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(out_ptr, rr + 1, 1)
    return np.cumsum(out_ptr), cc, vsum, rr


def _merge_self_loops_sorted(indptr, indices, data, rows, n):
    """``_merge_self_loops`` for a CSR whose columns already increase strictly in every row
    (no duplicates to sum): the same arrays without the sorts -- the diagonal entry of row i
    becomes a_ii + 1 in place, or a 1 inserted after the row's entries left of column i; then
    the exact zeros are pruned.  Linear time, so the products-scale parity tests do not spend
    minutes sorting 126 M keys that are sorted already."""
    nnz = indices.size
    on_diag = indices == rows
    has_diag = np.zeros(n, dtype=bool)
    has_diag[rows[on_diag]] = True
    ins = ~has_diag  # rows that get an inserted 1
    out_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.diff(indptr) + ins, out=out_ptr[1:])
    # an entry moves right by one when its row gets an insert to its left
    pos = out_ptr[rows] + (np.arange(nnz, dtype=np.int64) - indptr[rows])
    pos += (indices > rows) & ins[rows]
    left = np.bincount(rows[indices < rows], minlength=n).astype(np.int64)
    total = int(out_ptr[-1])
    cc = np.empty(total, dtype=np.int64)
    v = np.empty(total, dtype=np.float64)
    rr = np.empty(total, dtype=np.int64)
    cc[pos], rr[pos] = indices, rows
    v[pos] = np.where(on_diag, data + 1.0, data)
    ins_rows = np.flatnonzero(ins)
    ipos = out_ptr[ins_rows] + left[ins_rows]
    cc[ipos], rr[ipos], v[ipos] = ins_rows, ins_rows, 1.0
    keep = v != 0.0
    if not keep.all():
        cc, v, rr = cc[keep], v[keep], rr[keep]
        out_ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rr, minlength=n), out=out_ptr[1:])
    return out_ptr, cc, v, rr


def calc_a_hat(adj, mode: str = "sym"):
    """Restates helpers.py:58-66.  ``adj`` is a scipy CSR (any float dtype).

    Returns a scipy CSR in fp64 with sorted indices.  Degree D_i is the weighted row sum of
    A+I in column order (helpers.py:60); sym value = (dinv_i * a_ij) * dinv_j with
    dinv = 1/sqrt(D) (helpers.py:61-63, evaluated left-to-right as scipy does); rw value =
    (1/D_i) * a_ij (helpers.py:64-66)."""
    adj = sp.csr_matrix(adj)
    n = adj.shape[0]
    ptr, col, val, row = _merge_self_loops(adj.indptr, adj.indices, adj.data, n)
    # sequential per-row sum in column order (scipy: csr_matvec with a ones vector)
    deg = np.zeros(n, dtype=np.float64)
    nonempty = ptr[1:] > ptr[:-1]
    if nonempty.any():
        deg[nonempty] = np.add.reduceat(val, ptr[:-1][nonempty])
    if mode == "sym":
        dinv = 1.0 / np.sqrt(deg)
        out = (dinv[row] * val) * dinv[col]
    elif mode == "rw":
        dinv = 1.0 / deg
        out = dinv[row] * val
    else:
        raise ValueError(f"unknown mode {mode!r}")
    return sp.csr_matrix((out, col, ptr), shape=(n, n))


def compute_ppr(adj, alpha: float, mode: str = "sym") -> np.ndarray:
    """Restates helpers.py:68-71: alpha * inv(I - (1-alpha) A_hat), dense fp64."""
    a_hat = calc_a_hat(adj, mode)
    n = a_hat.shape[0]
    inner = np.eye(n) - (1.0 - alpha) * a_hat.toarray()
    return alpha * np.linalg.inv(inner)


# --------------------------------------------------------------------------------------
# Propagation (the APPNP loop)
# --------------------------------------------------------------------------------------


def appnp_propagate(a_hat, H, K: int, alpha: float, p_drop: float = 0.0, seed: int = 0):
    """Z_0 = H; Z_{k+1} = (1-alpha) * (M_k o A_hat) Z_k + alpha H, fp64.

    M_k is the edge-keep mask of ``edge_keep_mask`` scaled by 1/(1-p) (p_drop > 0 only)."""
    a_hat = sp.csr_matrix(a_hat, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    Z = H.copy()
    for k in range(K):
        if p_drop > 0.0:
            M = masked_operator(a_hat, k, p_drop, seed)
        else:
            M = a_hat
        Z = (1.0 - alpha) * (M @ Z) + alpha * H
    return Z


def appnp_backward(a_hat, dZ, K: int, alpha: float, p_drop: float = 0.0, seed: int = 0):
    """Adjoint of ``appnp_propagate`` w.r.t. H (dH = J^T dZ), fp64.

    G_K = dZ; dH = alpha G_K; G_k = (1-alpha) M_k^T G_{k+1} (k = K-1..0); dH += alpha G_k for
    k >= 1 and dH += G_0 at the end."""
    a_hat = sp.csr_matrix(a_hat, dtype=np.float64)
    G = np.asarray(dZ, dtype=np.float64).copy()
    if K == 0:
        return G
    dH = alpha * G
    for k in range(K - 1, -1, -1):
        M = masked_operator(a_hat, k, p_drop, seed) if p_drop > 0.0 else a_hat
        G = (1.0 - alpha) * (M.T @ G)
        dH = dH + (alpha * G if k >= 1 else G)
    return dH


def appnp_closed_form(a_hat, H, K: int, alpha: float):
    """Z_K = [alpha sum_{k<K} ((1-alpha)A)^k + ((1-alpha)A)^K] H."""
    a_hat = sp.csr_matrix(a_hat, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    term = H.copy()
    acc = alpha * term if K > 0 else np.zeros_like(H)
    for k in range(1, K):
        term = (1.0 - alpha) * (a_hat @ term)
        acc = acc + alpha * term
    term = (1.0 - alpha) * (a_hat @ term) if K > 0 else term
    return acc + term


def ppnp_forward(ppr, H, idx=None, ppr_sub=None):
    """Restates the propagation step of model.py:61-67 (``ppr[idx] @ H`` / ``ppr @ H``)."""
    if idx is not None:
        return np.asarray(ppr)[np.asarray(idx)] @ H
    if ppr_sub is not None:
        return np.asarray(ppr_sub) @ H
    raise Exception()


# --------------------------------------------------------------------------------------
# CPU baseline: the "reference's own CPU torch.sparse.mm path" named by north_star
# --------------------------------------------------------------------------------------


def torch_sparse_operator(a_hat):
    """fp32 torch CSR tensor of A_hat (CPU)."""
    import torch

    a = sp.csr_matrix(a_hat)
    return torch.sparse_csr_tensor(
        torch.from_numpy(a.indptr.astype(np.int64)),
        torch.from_numpy(a.indices.astype(np.int64)),
        torch.from_numpy(a.data.astype(np.float32)),
        size=a.shape,
    )


def appnp_propagate_torch_cpu(a_csr_t, H_t, K: int, alpha: float):
    """fp32 CPU torch.sparse.mm APPNP loop (SURVEY.md section 8(d) CPU baseline (i))."""
    import torch

    Z = H_t
    aH = alpha * H_t
    for _ in range(K):
        Z = torch.sparse.mm(a_csr_t, Z).mul_(1.0 - alpha).add_(aH)
    return Z


# --------------------------------------------------------------------------------------
# Edge dropout mask (counter hash; identical arithmetic to ppnp_amd/csrc/appnp_common.h)
# --------------------------------------------------------------------------------------

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _splitmix64(x):
    x = (x + _GOLDEN) & _M64 if isinstance(x, int) else (x + np.uint64(_GOLDEN))
    if isinstance(x, int):
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
        return x ^ (x >> 31)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def drop_threshold(p_drop: float) -> int:
    """24-bit threshold: an edge is dropped when its 24-bit hash < threshold.  p crosses the
    C ABI as a float, so the threshold is taken from float32(p) (0.3 -> 5033165, where the
    double 0.3 would give 5033164)."""
    p = float(np.float32(min(max(p_drop, 0.0), 1.0)))
    return int(p * (1 << 24))


def edge_keep_mask(rows, cols, k: int, p_drop: float, seed: int):
    """Boolean keep-mask for edges (row, col) at iteration k.  Keyed on (seed, k, row, col)
    only, so it is independent of partitioning and of the order edges are visited."""
    with np.errstate(over="ignore"):
        base = _splitmix64((seed + (k + 1) * _GOLDEN) & _M64)
        x = (np.asarray(rows, dtype=np.uint64) << np.uint64(32)) | np.asarray(
            cols, dtype=np.uint64
        )
        h = _splitmix64(x ^ np.uint64(base))
    u24 = (h >> np.uint64(40)).astype(np.int64)
    return u24 >= drop_threshold(p_drop)


def masked_operator(a_hat, k: int, p_drop: float, seed: int):
    """(M_k o A_hat) / (1-p) with the device mask (fp64 values; the 1/(1-p) factor is the
    fp32 value the kernel uses)."""
    a = sp.csr_matrix(a_hat, dtype=np.float64)
    n = a.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(a.indptr))
    keep = edge_keep_mask(rows, a.indices, k, p_drop, seed)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop)))
    data = np.where(keep, a.data * scale, 0.0)
    return sp.csr_matrix((data, a.indices, a.indptr), shape=a.shape)


# --------------------------------------------------------------------------------------
# Graph preprocessing (sparsegraph.py) and synthetic graphs
# --------------------------------------------------------------------------------------


def standardize(adj, select_lcc: bool = True):
    """Restates SparseGraph.standardize (sparsegraph.py:191-222) on the adjacency only:
    unweighted (135-138), undirected (112-128), no self-loops (380-395), LCC (355-377).
    Returns (adj_csr_fp32, kept_node_index)."""
    a = sp.csr_matrix(adj, dtype=np.float32)
    a.sum_duplicates()
    a.data = np.ones_like(a.data)
    a = ((a + a.T) > 0).astype(np.float32).tocsr()
    a.setdiag(0)
    a.eliminate_zeros()
    keep = np.arange(a.shape[0])
    if select_lcc:
        _, comp = csgraph.connected_components(a)
        sizes = np.bincount(comp)
        big = np.argsort(sizes)[::-1][:1]
        keep = np.nonzero(np.isin(comp, big))[0]
        a = a[keep][:, keep].tocsr()
    a.sort_indices()
    return a, keep


def synth_graph(n_nodes: int, n_edges: int, seed: int):
    """Uniform random undirected graph of SURVEY.md section 8(d): m (src, dst) pairs drawn
    uniformly, A = A + A^T, data := 1, no self loops.  Isolated nodes are kept."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n_nodes, size=n_edges, dtype=np.int64)
    dst = rng.integers(0, n_nodes, size=n_edges, dtype=np.int64)
    a = sp.coo_matrix(
        (np.ones(n_edges, dtype=np.float32), (src, dst)), shape=(n_nodes, n_nodes)
    ).tocsr()
    a = a + a.T
    a.data = np.ones_like(a.data)
    a.setdiag(0)
    a.eliminate_zeros()
    a.sort_indices()
    return a.astype(np.float32)


# --------------------------------------------------------------------------------------
# bf16 storage reference: what one step of the kernel may store, element by element
# --------------------------------------------------------------------------------------
#
# The kernel computes t = s * sum_j w_ij z_j + a * h_i in fp32 along some summation order, so
# its value before the store is within the standard (d + 2) 2^-24 S of the exact t, with
# S = s * sum_j |w_ij| |z_j| + a |h_i| and d the stored entries of the row.  ``delta`` is that
# with more than 2x headroom, (d + 8) 2^-23 S, which also leaves room for the fp32 dropout scale
# and the adjoint's extra factor.  Round-to-nearest-even then adds at most half a bf16 spacing of
# the value rounded, which lies within delta of t.  No figure here is measured on a device.


def round_bf16(x):
    """float32 -> float32 holding bf16 values: round to nearest even, NaN kept (quiet).  The
    integer trick of ``f32_to_bf16`` in ppnp_amd/csrc/appnp_device.h."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    with np.errstate(over="ignore"):
        r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)
    r = np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), r).astype(np.uint32)
    return (r << np.uint32(16)).view(np.float32).reshape(x.shape)


def spacing_bf16(x):
    """2^(floor(log2(max(|x|, 2^-126))) - 7): the distance between neighbouring bf16 values in
    the binade of x (fp64)."""
    ax = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    _, e = np.frexp(ax)  # ax = m 2^e with m in [0.5, 1): floor(log2 ax) = e - 1
    return np.ldexp(1.0, e - 1 - 7)


def _step_operator(indptr, indices, w32, alpha, k, p_drop, seed, transposed, h_weight,
                   y_weight, row_lo=0):
    """The fp32 quantities of one kernel step, held in fp64: (indptr, indices, kept weights),
    s and a.  The dropout mask is keyed on global rows: row_lo + local row."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    w = np.asarray(w32, dtype=np.float32)
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr)) + row_lo
    if p_drop > 0.0:
        keep = (edge_keep_mask(indices, rows, k, p_drop, seed) if transposed
                else edge_keep_mask(rows, indices, k, p_drop, seed))
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop))
        w = np.where(keep, (w * scale).astype(np.float32), np.float32(0.0))
    s = float(np.float32(1.0) - np.float32(alpha))
    if y_weight is not None:
        s *= float(np.float32(y_weight))
    a = float(np.float32(alpha if h_weight is None else h_weight))
    return indptr, indices, w.astype(np.float64), s, a


def step_exact(indptr, indices, w32, Zin, H, alpha, k, p_drop, seed, transposed=False,
               h_weight=None, y_weight=None, row_lo=0):
    """One step of the kernel in exact arithmetic on the kernel's own fp32 operands.

    Returns (t, delta), fp64: t_i = s sum_j w_ij z_j + a h_i and delta_i = (d_i + 8) 2^-23 S_i,
    S_i = s sum_j |w_ij| |z_j| + a |h_i|, d_i the stored entries of row i.  s = float32(1) -
    float32(alpha) evaluated in fp32 as the library does, a = float32(alpha); ``w32`` are the
    fp32 A_hat values (``Graph.csr()``).  Under dropout the kept weights are float32(w32 *
    float32(1 / (1 - p))) with the mask of ``edge_keep_mask``; ``transposed`` keys entry (i, j)
    as (j, i) (the adjoint's rows are the forward's columns).  ``h_weight`` overrides a (the
    adjoint's last step adds dH with weight 1), ``y_weight`` multiplies s (the adjoint's earlier
    steps add alpha y to dH).  ``H`` may be None (a partial product).  ``row_lo``: global index
    of row 0 of ``indptr`` (the mask is keyed on global rows)."""
    indptr, indices, w, s, a = _step_operator(indptr, indices, w32, alpha, k, p_drop, seed,
                                              transposed, h_weight, y_weight, row_lo)
    Z = np.asarray(Zin, dtype=np.float64)
    n_rows = indptr.size - 1
    W = sp.csr_matrix((w, indices, indptr), shape=(n_rows, Z.shape[0]))
    t = s * (W @ Z)
    S = s * (abs(W) @ np.abs(Z))
    if H is not None:
        h = np.asarray(H, dtype=np.float64)
        t = t + a * h
        S = S + abs(a) * np.abs(h)
    d = np.diff(indptr).astype(np.float64)[:, None]
    return t, (d + 8.0) * 2.0 ** -23 * S


def close_bf16_step(out, t, delta, label=""):
    """Assert |out - t| <= 0.5 spacing_bf16(|t| + delta) + delta for every element; print and
    return (worst ratio, share of elements bit-equal to round_bf16(t))."""
    out = np.asarray(out, dtype=np.float64)
    bound = 0.5 * spacing_bf16(np.abs(t) + delta) + delta
    ratio = np.abs(out - t) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    rne = round_bf16(t.astype(np.float32)).astype(np.float64)
    share = float((out == rne).mean()) if out.size else 1.0
    over = int((~(ratio <= 1.0)).sum())  # a NaN in out counts as over
    print(f"bf16 step {label}: worst ratio {worst:.4f}, over the bound {over} of {out.size}, "
          f"bit-equal to RNE(t) {100.0 * share:.3f} %")
    if over:
        bad = np.argwhere(~(ratio <= 1.0))
        where = ", ".join(f"{tuple(i)} got {out[tuple(i)]:.6g} exact {t[tuple(i)]:.6g}"
                          for i in bad[:6])
        raise AssertionError(
            f"{over} of {out.size} elements beyond half a bf16 spacing + delta (worst ratio "
            f"{worst:.4f}) {label}: {len(set(bad[:, 0].tolist()))} rows, columns "
            f"{sorted(set(bad[:, -1].tolist()))[:16]}; {where}")
    return worst, share


def envelope(indptr, indices, w32, E_prev, E_h, t, delta, alpha, k=0, p_drop=0.0, seed=0,
             transposed=False, h_weight=None, y_weight=None, row_lo=0):
    """Elementwise bound on the difference of the next iterate of two faithful implementations
    (each rounds an fp32-accurate value to the nearest bf16) whose inputs differ by at most
    E_prev (the gathered operand) and E_h (the added one): rho + spacing_bf16(|t| + rho) with
    rho = s |A| E_prev + a E_h + delta, since |RNE(x) - RNE(y)| <= |x - y| + one spacing.  t and
    delta are ``step_exact`` on one implementation's inputs; delta's headroom over the standard
    bound covers the other's slightly different S (E_prev is a few bf16 spacings)."""
    indptr, indices, w, s, a = _step_operator(indptr, indices, w32, alpha, k, p_drop, seed,
                                              transposed, h_weight, y_weight, row_lo)
    E_prev = np.asarray(E_prev, dtype=np.float64)
    W = sp.csr_matrix((np.abs(w), indices, indptr), shape=(indptr.size - 1, E_prev.shape[0]))
    rho = s * (W @ E_prev) + delta
    if E_h is not None:
        rho = rho + abs(a) * np.asarray(E_h, dtype=np.float64)
    return rho + spacing_bf16(np.abs(t) + rho)
