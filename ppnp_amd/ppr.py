"""Rows of the PPR matrix for minibatch training, without the dense N x N inverse.

Reference: batch-main.py:111-117 forms the dense ``compute_ppr`` (helpers.py:68-71),
sparsifies it with ``topk`` and indexes ``model.ppr[idx_batch]`` per minibatch
(batch-main.py:140-146).  Here the rows come from the APPNP propagation of one-hot columns:

* sym:  Pi = alpha (I - (1-alpha) A_hat)^-1 is symmetric (A_hat is), so
        Pi[idx, :] = (Pi e_idx)^T = APPNP_K(E_idx)^T
* rw:   Pi^T = D Pi D^-1 (A symmetric), so Pi[i, :] = D * APPNP_K(e_i) / d_i

with E_idx the N x B one-hot matrix; the K-step series converges to the exact rows
(``tests/test_gpu_parity.py::test_ppr_rows_match_compute_ppr``).  The propagation is the
same fused HIP kernel, with F = B columns.

``batch_topk_quirk`` reproduces batch-main.py:115-116 literally, including its broadcasting
quirk (``ppr < thresh[:, -1]`` compares entry (i, j) with the threshold of row j, so each
COLUMN keeps its top k).  It needs every row's k-th largest value,
i.e. all of Pi, which it streams in column chunks: O(N^2) work, small graphs only -- exactly
the reference's own limit.

``topk_rows`` / ``sparsified_ppr`` are the same protocol without the N x N matrix: PPR columns
for a chunk of source nodes (``ppr_columns``), reduced on the device to each column's k largest
entries by ``ops.topk_columns`` (``appnp_topk_columns``), kept as a device CSR (``SparsePPR``).
``SparsePPR.batch`` is the minibatch wrapper batch-main.py:136-138 asks for; with
``slicer="device"`` the slice and its transpose come from ``ops.csr_batch`` (HIP kernels, one
24-byte read-back per batch) instead of torch operations, bit for bit the same.

The columns come from one of three routes: the K-step series (default), the Chebyshev solver
(``tol=``), or local forward push (``eps=``, ``ops.push_columns``: work per source that follows
1 / eps and the source's neighbourhood instead of N -- the route for large graphs).  Everything
after the columns is the same for all three.  With ``eps=`` and ``select="lists"`` there are no
columns at all: ``ops.push_topk`` selects each source's top k straight from the nodes its push
took, all sources in one call, and returns the same rows bit for bit.
"""

from __future__ import annotations

import torch

from .graph import Graph
from .ops import (csr_batch, propagate_forward, push_columns, push_topk, solve_forward,
                  solve_iterations, topk_columns)
from .sparse import SparseFeatures


def _degrees(graph: Graph):
    """D_i of A+I from the stored inverse degrees (rw: dinv = 1/D)."""
    _, _, _, dinv = graph.csr()
    return 1.0 / dinv


def _one_route(tol, eps):
    if tol is not None and eps is not None:
        raise ValueError("tol= (the solver's columns) and eps= (forward push) are mutually "
                         "exclusive")


def _lists(select, eps) -> bool:
    """True for select="lists" (ops.push_topk: the top k straight from the push, one call for all
    sources); it needs the forward-push route."""
    if select not in ("block", "lists"):
        raise ValueError(f"select must be 'block' or 'lists', got {select!r}")
    if select == "lists" and eps is None:
        raise ValueError("select='lists' selects from the forward push's lists: it needs eps=")
    return select == "lists"


def ppr_columns(graph: Graph, idx: torch.Tensor, K: int = 10, alpha: float = 0.1,
                tol: float | None = None, eps: float | None = None, max_rounds: int = 1000,
                info: list | None = None):
    """Pi[:, idx] (N x B, fp32) = APPNP_K of the one-hot columns of idx; with ``tol`` the exact
    columns to that relative tolerance by the Chebyshev solver (ops.solve_forward), K ignored;
    with ``eps`` the forward-push columns (ops.push_columns: |error| < eps sqrt(d_j) for sym, eps
    for rw), K ignored.  ``tol`` and ``eps`` are mutually exclusive.  ``info``: a list that
    receives the push's ``(rounds, left)`` device tensors (``left`` all zero: the bound holds)."""
    _one_route(tol, eps)
    idx = torch.as_tensor(idx, device=graph.device).long()
    if eps is not None:
        X, rounds, left = push_columns(graph, idx, alpha, eps, max_rounds)
        if info is not None:
            info.append((rounds, left))
        return X
    B = int(idx.numel())
    E = torch.zeros(graph.n, B, dtype=torch.float32, device=graph.device)
    E[idx, torch.arange(B, device=graph.device)] = 1.0
    if tol is not None:
        return solve_forward(graph, E, solve_iterations(alpha, tol), alpha)
    return propagate_forward(graph, E, K, alpha)


def ppr_rows(graph: Graph, idx, K: int = 10, alpha: float = 0.1, topk: int | None = None,
             tol: float | None = None):
    """Pi[idx, :] as a dense B x N fp32 tensor (entries outside each row's top-k zeroed when
    ``topk`` is given).  ``tol``: as for ``ppr_columns``."""
    if not graph.symmetric:
        raise ValueError("ppr_rows needs an undirected graph (symmetric A)")
    idx = torch.as_tensor(idx, device=graph.device).long()
    cols = ppr_columns(graph, idx, K, alpha, tol)  # N x B
    if graph.mode == "sym":
        rows = cols.t().contiguous()
    else:  # rw: Pi[i, :] = D * Pi[:, i] / d_i
        deg = _degrees(graph).float()
        rows = (cols * deg[:, None]).t() / deg[idx][:, None]
        rows = rows.contiguous()
    if topk is not None and topk < graph.n:
        thr = rows.topk(topk, dim=1).values[:, -1:]
        rows = torch.where(rows >= thr, rows, torch.zeros_like(rows))
    return rows


def dense_ppr(graph: Graph, K: int = 10, alpha: float = 0.1, chunk: int = 1024,
              tol: float | None = None) -> torch.Tensor:
    """All of Pi (N x N fp32), row chunks of ``ppr_rows``: the truncated series of
    compute_ppr (helpers.py:68-71), or with ``tol`` the solver's rows.  Small graphs only
    (materialises N x N)."""
    n = graph.n
    if n * n > 2**31:
        raise ValueError("dense_ppr materialises N x N: N too large")
    P = torch.empty(n, n, dtype=torch.float32, device=graph.device)
    for s in range(0, n, chunk):
        idx = torch.arange(s, min(n, s + chunk), device=graph.device)
        P[s:s + len(idx)] = ppr_rows(graph, idx, K, alpha, tol=tol)
    return P


def batch_topk_quirk(graph: Graph, topk: int, K: int = 10, alpha: float = 0.1,
                     chunk: int = 1024) -> torch.Tensor:
    """Dense sparsified Pi exactly as batch-main.py:115-116 builds it:
    ``thresh, _ = ppr.topk(k, axis=-1); ppr[ppr < thresh[:, -1]] = 0`` (column-wise top-k
    through broadcasting).  Small graphs only (materialises N x N)."""
    P = dense_ppr(graph, K, alpha, chunk)
    thresh, _ = P.topk(topk, dim=-1)
    P[P < thresh[:, -1]] = 0
    return P


class SparsePPR(SparseFeatures):
    """Rows of a (sparsified) PPR matrix as a device CSR, ``shape = (rows, N)``: the sparse
    stand-in for the reference model's dense ``ppr`` buffer.  ``model(X, ppr=P)`` multiplies it
    through ``sparse_linear`` (``appnp_spmm``; the backward runs on the cached transpose)."""

    @classmethod
    def from_dense(cls, P: torch.Tensor) -> "SparsePPR":
        """The nonzero entries of a dense matrix, in canonical order."""
        nz = P != 0
        indptr = torch.zeros(P.shape[0] + 1, dtype=torch.int64, device=P.device)
        indptr[1:] = nz.sum(dim=1).cumsum(0)
        return cls(indptr, nz.nonzero()[:, 1], P[nz], P.shape, device=P.device)

    def _take(self, idx: torch.Tensor):
        """(entries per taken row, positions of their entries in ``indices`` / ``data``)."""
        idx = torch.as_tensor(idx, device=self.device).long()
        ip = self.indptr.long()
        start = ip[idx]
        lens = ip[idx + 1] - start
        off = lens.cumsum(0) - lens
        pos = torch.repeat_interleave(start - off, lens) + torch.arange(
            int(lens.sum()), device=self.device)
        return lens, pos

    @staticmethod
    def _indptr(lens: torch.Tensor) -> torch.Tensor:
        ip = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=lens.device)
        ip[1:] = lens.cumsum(0)
        return ip

    def rows(self, idx, slicer: str = "torch") -> "SparsePPR":
        """The rows ``idx`` (in that order) over all N columns: ``ppr[idx]``.

        ``slicer="device"``: the same matrix, bit for bit, from ``ops.csr_rows`` (HIP kernels, one
        16-byte read-back), with its ``_t`` set.  GPU matrices only."""
        if slicer not in ("torch", "device"):
            raise ValueError(f"slicer must be 'torch' or 'device', got {slicer!r}")
        if slicer == "device":
            if self.device.type != "cuda":
                raise ValueError("slicer='device' needs a matrix on a GPU (there is no CPU "
                                 "fallback); use slicer='torch'")
            return self._rows_device(idx)
        lens, pos = self._take(idx)
        return SparsePPR(self._indptr(lens), self.indices[pos], self.data[pos],
                         (lens.numel(), self.shape[1]), device=self.device)

    def batch(self, idx, slicer: str = "torch"):
        """batch-main.py:140-142 on the sparse form: ``ppr_sub = ppr[idx]``,
        ``sel = (ppr_sub > 0).any(dim=0)``, ``ppr_sub[:, sel]``.  Returns the
        [len(idx) x |sel|] SparsePPR with its columns relabelled into ``sel``, and ``sel`` as the
        sorted int64 column ids (index X with it: ``X[sel]``).

        ``slicer="device"``: the same matrix and ``sel``, bit for bit, from ``ops.csr_batch`` (HIP
        kernels, one 24-byte read-back per batch), which also emits the transpose: the
        sub-matrix's ``_t`` is set, so the backward of ``sparse_linear`` does not build it.  GPU
        matrices only."""
        if slicer not in ("torch", "device"):
            raise ValueError(f"slicer must be 'torch' or 'device', got {slicer!r}")
        if slicer == "device":
            if self.device.type != "cuda":
                raise ValueError("slicer='device' needs a matrix on a GPU (there is no CPU "
                                 "fallback); use slicer='torch'")
            indptr, indices, data, sel, t = csr_batch(self, idx)
            sub = SparsePPR(indptr, indices, data, (indptr.numel() - 1, int(sel.numel())),
                            device=self.device)
            sub._t = t
            return sub, sel
        lens, pos = self._take(idx)
        cols, vals = self.indices[pos].long(), self.data[pos]
        sel = torch.unique(cols[vals > 0])  # sorted
        new = torch.searchsorted(sel, cols).clamp_(max=max(int(sel.numel()) - 1, 0))
        keep = sel[new] == cols if sel.numel() else torch.zeros_like(cols, dtype=torch.bool)
        if not bool(keep.all()):  # a stored entry <= 0 in a column that no row selects
            row = torch.repeat_interleave(torch.arange(lens.numel(), device=self.device), lens)
            lens = torch.bincount(row[keep], minlength=lens.numel())
            new, vals = new[keep], vals[keep]
        sub = SparsePPR(self._indptr(lens), new, vals, (lens.numel(), int(sel.numel())),
                        device=self.device)
        return sub, sel


def _selected(graph: Graph, idx: torch.Tensor, k: int, K, alpha, tol, chunk, eps, max_rounds, info,
              lists: bool, rs=None, cs=None):
    """The flat ``(indices int32, values fp32)`` of the k selected entries of every source in
    ``idx``, source after source: ONE ``push_topk`` call (``lists``), or ``ppr_columns`` +
    ``topk_columns`` for ``chunk`` sources at a time.  ``rs`` [N] / ``cs`` [len(idx)]: the
    selection's row and column scales."""
    if not idx.numel():
        empty_i = torch.empty(0, dtype=torch.int32, device=graph.device)
        return empty_i, empty_i.float()
    if lists:
        i, v, rounds, left = push_topk(graph, idx, k, alpha, eps, max_rounds, rs, cs)
        if info is not None:
            info.append((rounds, left))
        return i.reshape(-1), v.reshape(-1)
    ix, dv = [], []
    for s in range(0, int(idx.numel()), int(chunk)):
        cols = ppr_columns(graph, idx[s:s + chunk], K, alpha, tol, eps, max_rounds, info)
        i, v = topk_columns(cols, k, rs, None if cs is None else cs[s:s + chunk])
        ix.append(i.reshape(-1))
        dv.append(v.reshape(-1))
    return torch.cat(ix), torch.cat(dv)


def topk_rows(graph: Graph, idx, k: int, K: int = 10, alpha: float = 0.1,
              tol: float | None = None, chunk: int = 128, eps: float | None = None,
              max_rounds: int = 1000, info: list | None = None,
              select: str = "block") -> SparsePPR:
    """Pi[idx, :] reduced to each row's k largest entries, as a SparsePPR [len(idx) x N] with
    exactly k entries per row (ties at the k-th value go to the smaller column).  The sources
    are taken ``chunk`` at a time: their PPR columns (``ppr_columns``: the K-step series, with
    ``tol`` the solver's columns, with ``eps`` the forward-push columns; ``max_rounds`` and
    ``info`` as there) are selected on the device by ``ops.topk_columns``, with
    no transposed copy and no read-back.  sym: the rows are the columns; rw:
    Pi[i, :] = D * Pi[:, i] / d_i, applied as the kernel's row and column scales.  Memory is
    one N x chunk block plus the len(idx) * k result.  Undirected graphs only.

    ``select="lists"`` (with ``eps``): the same rows, bit for bit, from ONE ``ops.push_topk`` call
    for all sources, which selects from the nodes each push took and forms no N x chunk block;
    ``chunk`` is not used and ``info`` receives one ``(rounds, left)`` pair."""
    if not graph.symmetric:
        raise ValueError("topk_rows needs an undirected graph (symmetric A)")
    _one_route(tol, eps)
    lists = _lists(select, eps)
    idx = torch.as_tensor(idx, device=graph.device).long()
    rs = cs_all = None
    if graph.mode != "sym":
        _, _, _, dinv = graph.csr()  # fp64 1 / D
        rs = (1.0 / dinv).float()
        cs_all = dinv[idx].float()
    ix, dv = _selected(graph, idx, k, K, alpha, tol, chunk, eps, max_rounds, info, lists, rs,
                       cs_all)
    B = int(idx.numel())
    indptr = torch.arange(B + 1, dtype=torch.int64, device=graph.device) * int(k)
    return SparsePPR(indptr, ix, dv, (B, graph.n), device=graph.device)


def sparsified_ppr(graph: Graph, k: int, K: int = 10, alpha: float = 0.1,
                   tol: float | None = None, chunk: int = 128, eps: float | None = None,
                   max_rounds: int = 1000, info: list | None = None,
                   select: str = "block") -> SparsePPR:
    """The sparsified Pi of batch-main.py:115-116 as an N x N SparsePPR, without the N x N
    matrix.  That line's broadcasting makes every COLUMN keep its top k,
    so the k largest entries of every column Pi[:, j] are selected chunk by chunk
    (``ppr_columns`` + ``ops.topk_columns``) as a CSC with exactly k entries per column, which
    ``appnp_csr_transpose`` turns into the CSR.  Memory is N * k entries (twice: the CSC stays
    as the cached transpose the backward needs) plus one N x chunk block; the N^2 guard of
    ``dense_ppr`` does not apply.  ``tol`` / ``eps`` / ``max_rounds`` / ``info``: the route to the
    columns, as for ``ppr_columns`` (``eps``: forward push, whose work does not grow with N).

    One deviation from the reference: it keeps every entry >= the threshold -- more than k on
    ties, and in practice sometimes fewer, because its fp64 inverse is not exactly symmetric and
    column j is compared with the threshold of ROW j.  This function keeps exactly k per column,
    by the kernel's tie rule (equal values: the smaller row index first).  For 'rw', where Pi is
    not symmetric, this is the column-wise reading as well.

    ``select="lists"`` (with ``eps``): the same CSC, bit for bit, from ONE ``ops.push_topk`` call
    over all N sources (no N x chunk block, a workspace that follows the slot count); ``chunk``
    is not used and ``info`` receives one ``(rounds, left)`` pair."""
    if not graph.symmetric:
        raise ValueError("sparsified_ppr needs an undirected graph (symmetric A)")
    _one_route(tol, eps)
    lists = _lists(select, eps)
    n = graph.n
    if n * int(k) >= 2**31:
        raise ValueError("sparsified_ppr: N * k exceeds the int32 CSR index range")
    ix, dv = _selected(graph, torch.arange(n, device=graph.device), k, K, alpha, tol, chunk, eps,
                       max_rounds, info, lists)
    indptr = torch.arange(n + 1, dtype=torch.int64, device=graph.device) * int(k)
    csc = SparsePPR(indptr, ix, dv, (n, n), device=graph.device)
    ip, jx, val = csc.transpose()
    P = SparsePPR(ip, jx, val, (n, n), device=graph.device)
    P._t = (csc.indptr, csc.indices, csc.data)  # the CSC is P^T: the backward's operand
    return P
