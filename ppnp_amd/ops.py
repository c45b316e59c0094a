"""APPNP propagation op on the gfx950 HIP kernels (no CPU fallback).

``propagate(graph, H, K, alpha)`` replaces the reference's propagation product
``self.ppr[idx] @ self.encoder(X)`` (/root/reference/model.py:63) by its K-truncated Neumann
series Z_K; ``Z_K[idx]`` is the drop-in for ``ppr[idx] @ H`` and
converges to it as K grows (K=100: 6e-7 max-abs on Cora-ML).

All calls are stream-ordered on ``torch.cuda.current_stream()``.
"""

from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .graph import Graph

_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def _check_dense(name, t, graph: Graph, rows: int):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device != graph.device:
        raise ValueError(f"{name} is on {t.device}, graph on {graph.device}")
    if t.dtype not in _DTYPES:
        raise TypeError(f"{name} dtype {t.dtype} unsupported (float32 / bfloat16)")
    if t.dim() != 2 or t.shape[0] != rows:
        raise ValueError(f"{name} must be [{rows}, F], got {tuple(t.shape)}")
    if t.shape[1] > 0 and t.stride(1) != 1:
        raise ValueError(f"{name} must have unit column stride")


def _ld(t) -> int:
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def _chain_call(fn_name: str, ws_bytes_of, name: str, X: torch.Tensor, graph: Graph, out,
                build_args) -> torch.Tensor:
    """One whole-graph propagation call of the library: ``fn_name`` from ``X`` (``name`` in the
    messages) into ``out``, or into a new contiguous tensor.  ``ws_bytes_of(lib, f, ld, dt)`` sizes
    the workspace allocated for the call; ``build_args(handle, X, Y, f, dt, ws, ws_bytes, stream)``
    returns the call's arguments."""
    _check_dense(name, X, graph, graph.n)
    Y = torch.empty_like(X, memory_format=torch.contiguous_format) if out is None else out
    _check_dense("out", Y, graph, graph.n)
    if Y.dtype != X.dtype or Y.shape != X.shape:
        raise ValueError(f"out must match {name} in shape and dtype")
    lib = _lib.load()
    dt = _DTYPES[X.dtype]
    f = int(X.shape[1])
    ws_bytes = int(ws_bytes_of(lib, f, _ld(Y), dt))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=graph.device) if ws_bytes else None
    with torch.cuda.device(graph.device):
        rc = getattr(lib, fn_name)(*build_args(graph.handle, X, Y, f, dt, ws, ws_bytes,
                                               _stream(graph.device)))
    _lib.check(fn_name, rc)
    return Y


def _chain_ws(graph: Graph, steps: int):
    """``appnp_workspace_bytes`` for a chain of ``steps`` steps; fewer than two need none."""
    return lambda lib, f, ld, dt: (lib.appnp_workspace_bytes(graph.handle, f, ld, dt)
                                   if steps >= 2 else 0)


def _chain_args(*params):
    """The argument order most chain calls share: the operands, ``params``, the workspace."""
    return lambda g, X, Y, f, dt, ws, ws_bytes, stream: (
        g, _vp(X), _ld(X), _vp(Y), _ld(Y), f, dt, *params, _vp(ws), ws_bytes, stream)


def propagate_forward(graph: Graph, H: torch.Tensor, K: int, alpha: float, p_drop: float = 0.0,
                      seed: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """Z = APPNP_K(H) via ``appnp_propagate`` (one fused HIP launch per iteration)."""
    return _chain_call("appnp_propagate", _chain_ws(graph, K), "H", H, graph, out,
                       _chain_args(int(K), float(alpha), float(p_drop), int(seed) & (2**64 - 1)))


def propagate_backward(graph: Graph, dZ: torch.Tensor, K: int, alpha: float, p_drop: float = 0.0,
                       seed: int = 0) -> torch.Tensor:
    """dH = J^T dZ via ``appnp_propagate_bwd`` (A_hat^T: A_hat itself for 'sym' on an
    undirected graph, else the transpose built with ``Graph(..., transpose=True)``)."""
    return _chain_call("appnp_propagate_bwd", _chain_ws(graph, K), "dZ", dZ.contiguous(), graph,
                       None,
                       _chain_args(int(K), float(alpha), float(p_drop), int(seed) & (2**64 - 1)))


# ---- torch.library registration ---------------------------------------------------------
# ``ppnp_amd::propagate`` / ``ppnp_amd::propagate_bwd`` are real dispatcher ops: torch.compile
# traces through them without a graph break (fake kernels give the output metadata), and
# autograd is registered on the op itself.  A custom op cannot take a Python object, so the
# graph crosses the dispatcher as the integer key Graph.key (graph.py registry).
# Call sites served: the three propagations per epoch of main.py:121, 138, 145.


@torch.library.custom_op("ppnp_amd::propagate", mutates_args=(), device_types="cuda")
def _propagate_op(H: torch.Tensor, graph_key: int, K: int, alpha: float, p_drop: float,
                  seed: int) -> torch.Tensor:
    return propagate_forward(Graph.lookup(graph_key), H.contiguous(), K, alpha, p_drop, seed)


@_propagate_op.register_fake
def _(H, graph_key, K, alpha, p_drop, seed):
    return torch.empty(H.shape, dtype=H.dtype, device=H.device)


@torch.library.custom_op("ppnp_amd::propagate_bwd", mutates_args=(), device_types="cuda")
def _propagate_bwd_op(dZ: torch.Tensor, graph_key: int, K: int, alpha: float, p_drop: float,
                      seed: int) -> torch.Tensor:
    return propagate_backward(Graph.lookup(graph_key), dZ, K, alpha, p_drop, seed)


@_propagate_bwd_op.register_fake
def _(dZ, graph_key, K, alpha, p_drop, seed):
    return torch.empty(dZ.shape, dtype=dZ.dtype, device=dZ.device)


def _propagate_setup(ctx, inputs, output):
    ctx.args = inputs[1:]


def _propagate_grad(ctx, dZ):
    return (torch.ops.ppnp_amd.propagate_bwd(dZ, *ctx.args), None, None, None, None, None)


_propagate_op.register_autograd(_propagate_grad, setup_context=_propagate_setup)


def propagate(graph: Graph, H: torch.Tensor, K: int = 10, alpha: float = 0.1,
              p_drop: float = 0.0, seed: int = 0) -> torch.Tensor:
    """Differentiable APPNP propagation Z_K(H) on the GPU (the ``ppnp_amd::propagate`` op).
    The seed is taken mod 2^64 like everywhere else (propagate_forward, the oracle); it crosses
    the op's int64 schema reinterpreted as signed, and propagate_forward maps it back."""
    s = int(seed) & (2**64 - 1)
    return torch.ops.ppnp_amd.propagate(H, graph.key, int(K), float(alpha), float(p_drop),
                                        s - 2**64 if s >= 2**63 else s)


# ---- exact PPNP: the Chebyshev solver (appnp_solve) ---------------------------------------


def solve_iterations(alpha: float = 0.1, tol: float = 1e-6) -> int:
    """Steps the solver takes for ``tol`` (``appnp_solve_iterations``): the smallest m with
    2 sigma^m / (1 + sigma^2m) <= tol, sigma = rho / (1 + sqrt(1 - rho^2)), rho = 1 - alpha
    (alpha = 0.1: 27 / 32 / 36 for 1e-5 / 1e-6 / 1e-7).  Host only."""
    m = C.c_int()
    _lib.check("appnp_solve_iterations",
               _lib.load().appnp_solve_iterations(float(alpha), float(tol), C.byref(m)))
    return m.value


def solve_weights(alpha: float, iters: int) -> list[float]:
    """The Chebyshev weights w_1 .. w_iters in fp64 (``appnp_solve_weights``).  Host only."""
    w = (C.c_double * max(int(iters), 1))()
    _lib.check("appnp_solve_weights", _lib.load().appnp_solve_weights(float(alpha), int(iters), w))
    return list(w)


def solve_forward(graph: Graph, H: torch.Tensor, iters: int, alpha: float,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Z = Pi H after ``iters`` Chebyshev steps via ``appnp_solve`` (one fused HIP launch per
    step).  fp32, undirected graphs, whole rows; see include/ppnp_amd.h."""
    return _chain_call("appnp_solve", _chain_ws(graph, iters), "H", H, graph, out,
                       _chain_args(int(iters), float(alpha)))


def solve_backward(graph: Graph, dZ: torch.Tensor, iters: int, alpha: float) -> torch.Tensor:
    """dH = Pi^T dZ via ``appnp_solve_bwd``: the same solve on A_hat^T, i.e. the gradient of the
    converged operator (rw needs ``Graph(..., transpose=True)``)."""
    return _chain_call("appnp_solve_bwd", _chain_ws(graph, iters), "dZ", dZ.contiguous(), graph,
                       None, _chain_args(int(iters), float(alpha)))


@torch.library.custom_op("ppnp_amd::solve", mutates_args=(), device_types="cuda")
def _solve_op(H: torch.Tensor, graph_key: int, iters: int, alpha: float) -> torch.Tensor:
    return solve_forward(Graph.lookup(graph_key), H.contiguous(), iters, alpha)


@_solve_op.register_fake
def _(H, graph_key, iters, alpha):
    return torch.empty(H.shape, dtype=H.dtype, device=H.device)


@torch.library.custom_op("ppnp_amd::solve_bwd", mutates_args=(), device_types="cuda")
def _solve_bwd_op(dZ: torch.Tensor, graph_key: int, iters: int, alpha: float) -> torch.Tensor:
    return solve_backward(Graph.lookup(graph_key), dZ, iters, alpha)


@_solve_bwd_op.register_fake
def _(dZ, graph_key, iters, alpha):
    return torch.empty(dZ.shape, dtype=dZ.dtype, device=dZ.device)


def _solve_setup(ctx, inputs, output):
    ctx.args = inputs[1:]


def _solve_grad(ctx, dZ):
    return (torch.ops.ppnp_amd.solve_bwd(dZ, *ctx.args), None, None, None)


_solve_op.register_autograd(_solve_grad, setup_context=_solve_setup)


def solve(graph: Graph, H: torch.Tensor, alpha: float = 0.1, tol: float = 1e-6,
          iters: int | None = None) -> torch.Tensor:
    """Differentiable exact PPNP propagation Pi H, Pi = alpha (I - (1-alpha) A_hat)^-1, to the
    relative tolerance ``tol`` (the ``ppnp_amd::solve`` op): ``solve_iterations(alpha, tol)``
    Chebyshev steps unless ``iters`` is given.  fp32 H on an undirected graph."""
    m = solve_iterations(alpha, tol) if iters is None else int(iters)
    return torch.ops.ppnp_amd.solve(H, graph.key, m, float(alpha))


# ---- polynomial propagation with device coefficients (appnp_poly) --------------------------

POLY_MAX_K = 1024  # APPNP_POLY_MAX_K of include/ppnp_amd.h


def ppr_coefficients(K: int, alpha: float, device=None) -> torch.Tensor:
    """gamma of the K-step APPNP series, fp32 [K + 1]: alpha (1-alpha)^k for k < K and
    (1-alpha)^K last (they sum to 1), so ``poly(graph, H, gamma) == propagate(graph, H, K, alpha)``
    up to rounding.  Computed in fp64."""
    K, alpha = int(K), float(alpha)
    g = torch.tensor([alpha * (1.0 - alpha) ** k for k in range(K)] + [(1.0 - alpha) ** K],
                     dtype=torch.float64).float()
    return g.to(device) if device is not None else g


def heat_coefficients(K: int, t: float, device=None) -> torch.Tensor:
    """gamma of heat-kernel diffusion truncated at K, fp32 [K + 1]: e^-t t^k / k!.  Computed in
    fp64."""
    k = torch.arange(int(K) + 1, dtype=torch.float64)
    g = torch.exp(-float(t) + k * math.log(float(t)) - torch.lgamma(k + 1)) if t > 0 else \
        (k == 0).double()
    return g.float().to(device) if device is not None else g.float()


def _check_coef(coef, graph: Graph) -> int:
    if not torch.is_tensor(coef) or coef.dtype != torch.float32 or coef.dim() != 1:
        raise TypeError("coef must be a 1-D float32 tensor [K + 1]")
    if coef.device != graph.device:
        raise ValueError(f"coef is on {coef.device}, graph on {graph.device}: the kernels read it "
                         "in device memory")
    K = int(coef.numel()) - 1
    if K < 0 or K > POLY_MAX_K:
        raise ValueError(f"coef must hold 1 to {POLY_MAX_K + 1} coefficients, got {K + 1}")
    return K


def poly_forward(graph: Graph, H: torch.Tensor, coef: torch.Tensor,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Z = sum_k coef[k] A_hat^k H via ``appnp_poly`` (K = len(coef) - 1 fused HIP launches).
    ``coef`` stays on the device: nothing is read back.  fp32; see include/ppnp_amd.h."""
    _check_dense("H", H, graph, graph.n)  # before coef, as ever
    K = _check_coef(coef, graph)
    coef = coef.detach().contiguous()
    return _chain_call(
        "appnp_poly", lambda lib, f, ld, dt: lib.appnp_poly_workspace_bytes(graph.handle, f, K, 0),
        "H", H, graph, out, _chain_args(K, _vp(coef)))


def poly_backward(graph: Graph, dZ: torch.Tensor, H: torch.Tensor | None, coef: torch.Tensor,
                  need_dcoef: bool = True):
    """``(dH, dcoef)`` of ``poly_forward`` via ``appnp_poly_bwd``: dH = sum_k coef[k] (A_hat^T)^k dZ
    and, with ``need_dcoef``, dcoef[k] = <(A_hat^T)^k dZ, H> (fp32 [K + 1] on the device, bitwise
    reproducible); else dcoef is None and H is not read.  A_hat^T: A_hat itself for 'sym' on an
    undirected graph, else the transpose built with ``Graph(..., transpose=True)``."""
    _check_dense("dZ", dZ, graph, graph.n)
    K = _check_coef(coef, graph)
    coef = coef.detach().contiguous()
    if need_dcoef:
        _check_dense("H", H, graph, graph.n)
        if H.dtype != dZ.dtype or H.shape != dZ.shape:
            raise ValueError("H must match dZ in shape and dtype")
    dcoef = torch.empty(K + 1, dtype=torch.float32, device=graph.device) if need_dcoef else None
    if need_dcoef and dZ.numel() == 0:
        dcoef.zero_()  # an empty shape: the library has nothing to do
    dH = _chain_call(
        "appnp_poly_bwd",
        lambda lib, f, ld, dt: lib.appnp_poly_workspace_bytes(graph.handle, f, K,
                                                              int(bool(need_dcoef))),
        "dZ", dZ, graph, None,
        lambda g, X, Y, f, dt, ws, ws_bytes, stream: (
            g, _vp(X), _ld(X), _vp(H) if need_dcoef else None, _ld(H) if need_dcoef else 0,
            _vp(Y), _ld(Y), _vp(dcoef), f, dt, K, _vp(coef), _vp(ws), ws_bytes, stream))
    return dH, dcoef


@torch.library.custom_op("ppnp_amd::poly", mutates_args=(), device_types="cuda")
def _poly_op(H: torch.Tensor, coef: torch.Tensor, graph_key: int) -> torch.Tensor:
    return poly_forward(Graph.lookup(graph_key), H.contiguous(), coef)


@_poly_op.register_fake
def _(H, coef, graph_key):
    return torch.empty(H.shape, dtype=H.dtype, device=H.device)


@torch.library.custom_op("ppnp_amd::poly_bwd", mutates_args=(), device_types="cuda")
def _poly_bwd_op(dZ: torch.Tensor, H: torch.Tensor, coef: torch.Tensor, graph_key: int,
                 need_dcoef: bool) -> tuple[torch.Tensor, torch.Tensor]:
    dH, dcoef = poly_backward(Graph.lookup(graph_key), dZ.contiguous(), H.contiguous(), coef,
                              need_dcoef)
    return dH, dcoef if need_dcoef else coef.new_empty(0)


@_poly_bwd_op.register_fake
def _(dZ, H, coef, graph_key, need_dcoef):
    return (torch.empty(dZ.shape, dtype=dZ.dtype, device=dZ.device),
            coef.new_empty(coef.shape if need_dcoef else (0,)))


def _poly_setup(ctx, inputs, output):
    H, coef, ctx.graph_key = inputs
    ctx.save_for_backward(H, coef)


def _poly_grad(ctx, dZ):
    H, coef = ctx.saved_tensors
    need = bool(ctx.needs_input_grad[1])
    dH, dcoef = torch.ops.ppnp_amd.poly_bwd(dZ, H, coef, ctx.graph_key, need)
    return dH, (dcoef if need else None), None


_poly_op.register_autograd(_poly_grad, setup_context=_poly_setup)


def poly(graph: Graph, H: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """Differentiable polynomial propagation sum_k coef[k] A_hat^k H (the ``ppnp_amd::poly`` op),
    with gradients for H and for coef: GPR-GNN when coef is a parameter, APPNP with
    ``ppr_coefficients``, heat-kernel diffusion with ``heat_coefficients``.  ``coef``: fp32
    [K + 1] on the graph's device."""
    _check_coef(coef, graph)
    return torch.ops.ppnp_amd.poly(H, coef, graph.key)


# ---- sparse top-k PPR rows: the column selection (appnp_topk_columns) ----------------------


def _scales(row_scale, col_scale, n: int, b: int, device):
    """The selection's ``[row_scale, col_scale]`` (fp32 [n] / [b] on ``device``, or None), checked
    and contiguous."""
    scales = []
    for name, t, m in (("row_scale", row_scale, n), ("col_scale", col_scale, b)):
        if t is not None:
            if t.dtype != torch.float32 or t.device != device or tuple(t.shape) != (m,):
                raise ValueError(f"{name} must be float32 [{m}] on {device}")
            t = t.contiguous()
        scales.append(t)
    return scales


def topk_columns(X: torch.Tensor, k: int, row_scale: torch.Tensor | None = None,
                 col_scale: torch.Tensor | None = None):
    """The k largest entries of every column of X [n, b] (fp32, unit column stride, a padded
    leading dimension is passed through) via ``appnp_topk_columns``: ``(idx int32 [b, k],
    val fp32 [b, k])``, each row sorted by ascending index -- the rows of a canonical CSR with
    exactly k entries per row.  The candidate of (r, c) is ``(X[r, c] * row_scale[r]) *
    col_scale[c]``; ties go to the smaller index, NaN orders last.  Stream-ordered on the current
    stream, no host synchronisation, bitwise deterministic; see include/ppnp_amd.h."""
    if not torch.is_tensor(X) or X.dtype != torch.float32 or X.dim() != 2:
        raise TypeError("X must be a 2-D float32 tensor")
    if not X.is_cuda:
        raise ValueError("X must be a device tensor (there is no CPU fallback)")
    n, b = int(X.shape[0]), int(X.shape[1])
    if b > 0 and X.stride(1) != 1:
        raise ValueError("X must have unit column stride")
    k = int(k)
    if k < 1 or (n * b > 0 and k > n):
        raise ValueError(f"k must be in [1, {n}], got {k}")
    scales = _scales(row_scale, col_scale, n, b, X.device)
    idx = torch.empty(b, k, dtype=torch.int32, device=X.device)
    val = torch.empty(b, k, dtype=torch.float32, device=X.device)
    lib = _lib.load()
    ws_bytes = int(lib.appnp_topk_workspace_bytes(n, b, k))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=X.device) if ws_bytes else None
    with torch.cuda.device(X.device):
        rc = lib.appnp_topk_columns(_vp(X), _ld(X), n, b, k, _vp(scales[0]), _vp(scales[1]),
                                    _vp(idx), _vp(val), k, _vp(ws), ws_bytes, _stream(X.device))
    _lib.check("appnp_topk_columns", rc)
    return idx, val


# ---- PPR columns by local forward push (appnp_push_columns) --------------------------------


def _push_graph(fn: str, graph: Graph, rc: int | None = None):
    """What ``fn`` (push_columns / push_topk) asks of its graph.  Before the call (``rc`` None):
    undirected and not row-partitioned.  After it, with the call's return code: 'rw' without the
    transpose in words, anything else through ``_lib.check``."""
    if rc is None:
        if not graph.symmetric:
            raise ValueError(f"{fn} needs an undirected graph (symmetric A)")
        if graph.row_lo != 0 or graph.row_hi != graph.n:
            raise ValueError(f"{fn} needs a full (not row-partitioned) graph")
        return
    if rc == _lib.APPNP_ENOTSUP and graph.mode == "rw":
        raise ValueError(f"{fn} on an 'rw' graph walks A_hat^T: build the graph with "
                         "transpose=True (Graph.from_scipy(..., transpose=True))")
    _lib.check(f"appnp_{fn}", rc)


def push_columns(graph: Graph, idx, alpha: float = 0.1, eps: float = 1e-4,
                 max_rounds: int = 1000, out: torch.Tensor | None = None):
    """Pi[:, idx] by forward push via ``appnp_push_columns``: ``(X fp32 [n, B], rounds int32 [B],
    left int32 [B])``.  A source's residual is pushed only where it has reached ``eps * w_j``
    (w_j = sqrt(d_j) for 'sym', 1 for 'rw'), in int64 fixed point, so the work per source follows
    1 / eps and its neighbourhood, not n, and X is bitwise reproducible.  ``left[c] == 0`` means
    column c ended with an empty frontier and |Pi[j, s] - X[j, c]| < eps * w_j holds;
    ``left[c] > 0``: ``max_rounds`` cut it short; ``-1``: ``idx[c]`` lies outside [0, n) (a zero
    column).  ``out``: an fp32 [n, B] tensor with unit column stride to write into (a padded
    leading dimension is passed through, the padding is not touched).  Undirected full graphs;
    'rw' needs the transpose (``Graph.from_scipy(..., transpose=True)``).  Stream-ordered on the
    current stream, no host synchronisation; see include/ppnp_amd.h."""
    _push_graph("push_columns", graph)
    idx = torch.as_tensor(idx, device=graph.device).long().contiguous().reshape(-1)
    n, b = graph.n, int(idx.numel())
    X = torch.empty(n, b, dtype=torch.float32, device=graph.device) if out is None else out
    if X.dtype != torch.float32 or X.device != graph.device or tuple(X.shape) != (n, b):
        raise ValueError(f"out must be float32 [{n}, {b}] on {graph.device}")
    if b > 0 and n > 0 and X.stride(1) != 1:
        raise ValueError("out must have unit column stride")
    rounds = torch.zeros(b, dtype=torch.int32, device=graph.device)
    left = torch.zeros(b, dtype=torch.int32, device=graph.device)
    lib = _lib.load()
    ws_bytes = int(lib.appnp_push_workspace_bytes(n, b))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=graph.device) if ws_bytes else None
    with torch.cuda.device(graph.device):
        rc = lib.appnp_push_columns(graph.handle, _vp(idx), b, float(alpha), float(eps),
                                    int(max_rounds), _vp(X), max(_ld(X), b), _vp(rounds),
                                    _vp(left), _vp(ws), ws_bytes, _stream(graph.device))
    _push_graph("push_columns", graph, rc)
    return X, rounds, left


PUSH_TOPK_MAX_K = 1024  # APPNP_PUSH_TOPK_MAX_K of include/ppnp_amd.h


def push_topk_slots(graph: Graph, b: int) -> int:
    """The slot count ``push_topk`` picks for ``b`` sources: one workgroup per compute unit at
    the most, lowered until the workspace fits a quarter of the free device memory."""
    slots = max(1, min(int(b), torch.cuda.get_device_properties(graph.device).multi_processor_count))
    lib = _lib.load()
    budget = torch.cuda.mem_get_info(graph.device)[0] // 4
    one = int(lib.appnp_push_topk_workspace_bytes(graph.n, 1))
    two = int(lib.appnp_push_topk_workspace_bytes(graph.n, 2))
    per_slot = max(two - one, 1)
    if int(lib.appnp_push_topk_workspace_bytes(graph.n, slots)) > budget:
        slots = max(1, min(slots, (budget - one) // per_slot + 1))
    return slots


def push_topk(graph: Graph, idx, k: int, alpha: float = 0.1, eps: float = 1e-4,
              max_rounds: int = 1000, row_scale: torch.Tensor | None = None,
              col_scale: torch.Tensor | None = None, slots: int | None = None):
    """The k largest entries of the forward-push columns Pi[:, idx], straight from the nodes each
    push took, via ``appnp_push_topk``: ``(idx int32 [B, k], val fp32 [B, k], rounds int32 [B],
    left int32 [B])``, bit for bit what ``push_columns`` followed by ``topk_columns`` returns for
    the same arguments, without the dense [n, B] block: the cost per source follows the push, not
    n.  ``row_scale`` [n] / ``col_scale`` [B]: the selection's scales (finite and > 0).
    ``slots``: workgroups launched, each running every slots-th source on one reusable slice of
    the workspace (36 n bytes per slot); None picks ``push_topk_slots``.  One call takes any
    number of sources.  ``rounds`` / ``left`` and the graph requirements are ``push_columns``'s.
    Stream-ordered on the current stream, no host synchronisation; see include/ppnp_amd.h."""
    _push_graph("push_topk", graph)
    idx = torch.as_tensor(idx, device=graph.device).long().contiguous().reshape(-1)
    n, b = graph.n, int(idx.numel())
    k = int(k)
    if k < 1 or (n * b > 0 and k > n):
        raise ValueError(f"k must be in [1, {n}], got {k}")
    if k > PUSH_TOPK_MAX_K:
        raise ValueError(f"push_topk selects at most k = {PUSH_TOPK_MAX_K}, got {k}")
    scales = _scales(row_scale, col_scale, n, b, graph.device)
    if slots is None:
        slots = push_topk_slots(graph, b) if n * b > 0 else 1
    slots = int(slots)
    if slots < 1:
        raise ValueError(f"slots must be at least 1, got {slots}")
    out_idx = torch.empty(b, k, dtype=torch.int32, device=graph.device)
    out_val = torch.empty(b, k, dtype=torch.float32, device=graph.device)
    rounds = torch.zeros(b, dtype=torch.int32, device=graph.device)
    left = torch.zeros(b, dtype=torch.int32, device=graph.device)
    lib = _lib.load()
    ws_bytes = int(lib.appnp_push_topk_workspace_bytes(n, slots))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=graph.device) if ws_bytes else None
    with torch.cuda.device(graph.device):
        rc = lib.appnp_push_topk(graph.handle, _vp(idx), b, float(alpha), float(eps),
                                 int(max_rounds), k, _vp(scales[0]), _vp(scales[1]),
                                 _vp(out_idx), _vp(out_val), k, _vp(rounds), _vp(left), slots,
                                 _vp(ws), ws_bytes, _stream(graph.device))
    _push_graph("push_topk", graph, rc)
    return out_idx, out_val, rounds, left


# ---- the per-minibatch slice of a sparse PPR matrix (appnp_csr_batch_count / _emit) ---------

CSR_BATCH_SCAN_PASS = 4096  # APPNP_CSR_BATCH_SCAN_PASS of include/ppnp_amd.h
CSR_BATCH_LDS_COLS = 131072  # APPNP_CSR_BATCH_LDS_COLS


def csr_batch(P, idx):
    """batch-main.py:140-142 on a device CSR ``P`` (a ``SparseFeatures``: int32 ``indptr`` /
    ``indices``, fp32 ``data``, ``shape``) via ``appnp_csr_batch_count`` / ``_emit``: the rows
    ``idx`` (int64, any order, duplicates allowed) restricted to the columns ``sel`` in which one
    of them holds an entry > 0, relabelled into ``sel``.  Returns ``(indptr int32 [b + 1],
    indices int32, data fp32, sel int64 ascending, (t_indptr, t_indices, t_data))``: the
    [b x |sel|] CSR, bit for bit what ``SparsePPR.batch`` builds with torch, and the canonical
    CSR of its transpose, bit for bit ``appnp_csr_transpose`` of it.  One read-back per call (the
    three counts, 24 bytes) sizes the outputs; everything else is stream-ordered on the current
    stream.  ``IndexError`` for an index outside [0, rows), ``ValueError`` for 2^31 kept entries
    or more.  See include/ppnp_amd.h."""
    dev = P.device
    if dev.type != "cuda":
        raise ValueError("csr_batch needs a matrix on a GPU (there is no CPU fallback)")
    idx = torch.as_tensor(idx, device=dev).long().contiguous().reshape(-1)
    rows, cols = P.shape
    b = int(idx.numel())
    i32 = {"dtype": torch.int32, "device": dev}
    if b == 0 or cols == 0:  # nothing to select from: the library writes nothing
        out_indptr = torch.zeros(b + 1, **i32)
        if b and bool(((idx < 0) | (idx >= rows)).any()):
            raise IndexError(f"csr_batch: an index lies outside [0, {rows})")
        empty = torch.empty(0, **i32)
        return (out_indptr, empty, empty.float(), torch.empty(0, dtype=torch.int64, device=dev),
                (torch.zeros(1, **i32), empty.clone(), empty.float()))
    out_indptr = torch.empty(b + 1, **i32)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    lib = _lib.load()
    head = int(lib.appnp_csr_batch_workspace_bytes(cols, b, 0))
    ws = torch.empty(head, dtype=torch.uint8, device=dev)
    src = (_vp(P.indptr), _vp(P.indices), _vp(P.data), rows, cols, _vp(idx), b)
    with torch.cuda.device(dev):
        rc = lib.appnp_csr_batch_count(*src, _vp(out_indptr), _vp(counts), _vp(ws), head,
                                       _stream(dev))
    _lib.check("appnp_csr_batch_count", rc)
    nnz, n_sel, bad = counts.cpu().tolist()  # the one read-back: the shapes depend on the data
    if bad:
        raise IndexError(f"csr_batch: {bad} of {b} indices lie outside [0, {rows})")
    if nnz >= 2**31:
        raise ValueError(f"csr_batch: {nnz} kept entries exceed the int32 CSR index range")
    # the kept entries are known only now: emit's workspace starts with a copy of count's state
    need = int(lib.appnp_csr_batch_workspace_bytes(cols, b, nnz))
    if need > head:
        ws_emit = torch.empty(need, dtype=torch.uint8, device=dev)
        ws_emit[:head].copy_(ws)
        ws = ws_emit
    out_indices = torch.empty(nnz, **i32)
    out_vals = torch.empty(nnz, dtype=torch.float32, device=dev)
    sel = torch.empty(n_sel, dtype=torch.int64, device=dev)
    t_indptr = torch.empty(n_sel + 1, **i32)
    t_indices = torch.empty(nnz, **i32)
    t_vals = torch.empty(nnz, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.appnp_csr_batch_emit(*src, _vp(out_indptr), nnz, n_sel, _vp(out_indices),
                                      _vp(out_vals), _vp(sel), _vp(t_indptr), _vp(t_indices),
                                      _vp(t_vals), _vp(ws), int(ws.numel()), _stream(dev))
    _lib.check("appnp_csr_batch_emit", rc)
    return out_indptr, out_indices, out_vals, sel, (t_indptr, t_indices, t_vals)


def csr_rows(M, idx, transpose: bool = True):
    """``M[idx]`` on a device CSR ``M`` (a ``SparseFeatures``) via ``appnp_csr_rows_count`` /
    ``_emit``: the rows ``idx`` (int64, any order, duplicates allowed) copied whole, columns not
    relabelled, values bit for bit.  Returns ``(indptr int32 [b + 1], indices int32, data fp32,
    t)``; ``t`` is ``(t_indptr, t_indices, t_data)``, the canonical CSR [cols x b] of the
    transpose, bit for bit ``appnp_csr_transpose`` of the slice, or ``None`` with
    ``transpose=False`` (then emit is one launch: the route under ``no_grad``).  One read-back per
    call (the two counts, 16 bytes) sizes the outputs; everything else is stream-ordered on the
    current stream.  ``IndexError`` for an index outside [0, rows), ``ValueError`` for 2^31
    entries or more.  See include/ppnp_amd.h."""
    dev = M.device
    if dev.type != "cuda":
        raise ValueError("csr_rows needs a matrix on a GPU (there is no CPU fallback)")
    idx = torch.as_tensor(idx, device=dev).long().contiguous().reshape(-1)
    rows, cols = M.shape
    b = int(idx.numel())
    i32 = {"dtype": torch.int32, "device": dev}
    if b == 0:  # the library writes nothing
        empty = torch.empty(0, **i32)
        t = (torch.zeros(cols + 1, **i32), empty.clone(), empty.float()) if transpose else None
        return torch.zeros(1, **i32), empty, empty.float(), t
    out_indptr = torch.empty(b + 1, **i32)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    lib = _lib.load()
    src = (_vp(M.indptr), _vp(M.indices), _vp(M.data), rows, cols, _vp(idx), b)
    with torch.cuda.device(dev):
        rc = lib.appnp_csr_rows_count(*src, _vp(out_indptr), _vp(counts), _stream(dev))
    _lib.check("appnp_csr_rows_count", rc)
    nnz, bad = counts.cpu().tolist()  # the one read-back: the sizes depend on the data
    if bad:
        raise IndexError(f"csr_rows: {bad} of {b} indices lie outside [0, {rows})")
    if nnz >= 2**31:
        raise ValueError(f"csr_rows: {nnz} entries exceed the int32 CSR index range")
    out_indices = torch.empty(nnz, **i32)
    out_vals = torch.empty(nnz, dtype=torch.float32, device=dev)
    t, ws, need = None, None, 0
    if transpose:
        t = (torch.empty(cols + 1, **i32), torch.empty(nnz, **i32),
             torch.empty(nnz, dtype=torch.float32, device=dev))
        need = int(lib.appnp_csr_rows_workspace_bytes(cols, nnz))
        ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    tp = [_vp(x) for x in t] if transpose else [None, None, None]
    with torch.cuda.device(dev):
        rc = lib.appnp_csr_rows_emit(*src, _vp(out_indptr), nnz, _vp(out_indices), _vp(out_vals),
                                     *tp, _vp(ws), need, _stream(dev))
    _lib.check("appnp_csr_rows_emit", rc)
    return out_indptr, out_indices, out_vals, t


def step(graph: Graph, Zin: torch.Tensor, H: torch.Tensor, out: torch.Tensor, k: int,
         alpha: float, part: int = _lib.PART_ALL, partial: torch.Tensor | None = None,
         p_drop: float = 0.0, seed: int = 0) -> torch.Tensor:
    """One iteration on the held rows (``appnp_step``); Zin holds all n rows."""
    lib = _lib.load()
    _check_dense("Zin", Zin, graph, graph.n)
    dt = _DTYPES[Zin.dtype]
    f = int(Zin.shape[1])
    ld_h = _ld(H) if H is not None else 0
    ld_p = _ld(partial) if partial is not None else 0
    with torch.cuda.device(graph.device):
        rc = lib.appnp_step(graph.handle, int(part), _vp(Zin), _ld(Zin), _vp(H), ld_h, _vp(out),
                            _ld(out), _vp(partial), ld_p, f, dt, int(k), float(alpha),
                            float(p_drop), int(seed) & (2**64 - 1), _stream(graph.device))
    _lib.check("appnp_step", rc)
    return out


def shard_offsets(graph: Graph, nshards: int, shard_rows: int) -> None:
    """The held rows' entries grouped by source shard (``appnp_graph_shard_offsets``), for the
    pipelined row steps ``step_shards`` / ``step_split_shards``."""
    with torch.cuda.device(graph.device):
        rc = _lib.load().appnp_graph_shard_offsets(graph.handle, int(nshards), int(shard_rows),
                                                   _stream(graph.device))
    _lib.check("appnp_graph_shard_offsets", rc)


def step_shards(graph: Graph, s_lo: int, s_hi: int, mode: int, Zin: torch.Tensor,
                H: torch.Tensor | None, out: torch.Tensor | None, partial: torch.Tensor | None,
                k: int, alpha: float, p_drop: float = 0.0, seed: int = 0) -> None:
    """One iteration's product over source shards [s_lo, s_hi) of the held rows
    (``appnp_step_shards``): mode SHARDS_FIRST / _ACC into ``partial``, _LAST / _ONLY into
    ``out`` (fp32; Zin holds all n rows)."""
    _check_dense("Zin", Zin, graph, graph.n)
    f = int(Zin.shape[1])
    with torch.cuda.device(graph.device):
        rc = _lib.load().appnp_step_shards(
            graph.handle, int(s_lo), int(s_hi), int(mode), _vp(Zin), _ld(Zin), _vp(H),
            _ld(H) if H is not None else 0, _vp(out), _ld(out) if out is not None else 0,
            _vp(partial), _ld(partial) if partial is not None else 0, f, int(k), float(alpha),
            float(p_drop), int(seed) & (2**64 - 1), _stream(graph.device))
    _lib.check("appnp_step_shards", rc)


def step_split_shards(graph: Graph, s_lo: int, s_hi: int, mode: int,
                      zin_main: torch.Tensor | None, zin_rem: torch.Tensor | None,
                      H: torch.Tensor | None, f: int, k: int, alpha: float,
                      out_main: torch.Tensor | None = None, out_rem: torch.Tensor | None = None,
                      Z: torch.Tensor | None = None, partial: torch.Tensor | None = None,
                      p_drop: float = 0.0, seed: int = 0) -> None:
    """``step_shards`` on the split layout (``appnp_step_split_shards``): the main columns take
    the shard range and mode; _LAST / _ONLY then run the remainder pass."""
    with torch.cuda.device(graph.device):
        rc = _lib.load().appnp_step_split_shards(
            graph.handle, int(s_lo), int(s_hi), int(mode), _vp(zin_main), _vp(zin_rem), _vp(H),
            _ld(H) if H is not None else 0, _vp(out_main), _vp(out_rem), _vp(Z),
            _ld(Z) if Z is not None else 0, _vp(partial),
            _ld(partial) if partial is not None else 0, int(f), int(k), float(alpha),
            float(p_drop), int(seed) & (2**64 - 1), _stream(graph.device))
    _lib.check("appnp_step_split_shards", rc)


def split_copy(graph: Graph, H: torch.Tensor, main: torch.Tensor | None,
               rem: torch.Tensor) -> None:
    """Z_0 of the split layout on the held rows (``appnp_split_copy``): H [held rows, F] into
    rows [row_lo, row_hi) of the full-height parts main [*, fs] and rem [*, rem_width]."""
    with torch.cuda.device(graph.device):
        rc = _lib.load().appnp_split_copy(graph.handle, _vp(H), _ld(H), int(H.shape[1]),
                                          _vp(main), _vp(rem), _stream(graph.device))
    _lib.check("appnp_split_copy", rc)


def step_split(graph: Graph, part: int, zin_main: torch.Tensor | None, zin_rem: torch.Tensor,
               H: torch.Tensor | None, f: int, k: int, alpha: float,
               out_main: torch.Tensor | None = None, out_rem: torch.Tensor | None = None,
               Z: torch.Tensor | None = None, partial: torch.Tensor | None = None,
               p_drop: float = 0.0, seed: int = 0) -> None:
    """One iteration of the held rows on the split layout (``appnp_step_split``): from every row
    of zin_main / zin_rem into rows [row_lo, row_hi) of out_main / out_rem, or into Z (the held
    rows, all F columns) on the last iteration."""
    with torch.cuda.device(graph.device):
        rc = _lib.load().appnp_step_split(
            graph.handle, int(part), _vp(zin_main), _vp(zin_rem), _vp(H),
            _ld(H) if H is not None else 0, _vp(out_main), _vp(out_rem), _vp(Z),
            _ld(Z) if Z is not None else 0, _vp(partial),
            _ld(partial) if partial is not None else 0, int(f), int(k), float(alpha),
            float(p_drop), int(seed) & (2**64 - 1), _stream(graph.device))
    _lib.check("appnp_step_split", rc)


class PropagatePlan:
    """A captured propagation (``appnp_plan_create``): K launches recorded once into a hipGraph
    for fixed H / Z buffers, replayed with one graph launch.  Refill ``plan.H`` in place, call
    ``plan()``, read ``plan.Z``.  For small, launch-bound graphs and serving loops."""

    def __init__(self, graph: Graph, H: torch.Tensor, K: int = 10, alpha: float = 0.1,
                 p_drop: float = 0.0, seed: int = 0):
        self._capture("appnp_plan_create", graph, H,
                      (int(K), float(alpha), float(p_drop), int(seed) & (2**64 - 1)))

    def _capture(self, fn_name: str, graph: Graph, H: torch.Tensor, params: tuple):
        """Allocate Z and the workspace, then record ``fn_name`` on them with ``params``."""
        _check_dense("H", H, graph, graph.n)
        self.graph, self.H = graph, H
        self.Z = torch.empty_like(H, memory_format=torch.contiguous_format)
        lib = _lib.load()
        dt = _DTYPES[H.dtype]
        f = int(H.shape[1])
        self._ws_bytes = int(lib.appnp_workspace_bytes(graph.handle, f, _ld(self.Z), dt))
        self._ws = torch.empty(max(self._ws_bytes, 1), dtype=torch.uint8, device=graph.device)
        self._p = C.c_void_p()
        torch.cuda.current_stream(graph.device).synchronize()  # buffers allocated before capture
        with torch.cuda.device(graph.device):
            rc = getattr(lib, fn_name)(graph.handle, _vp(H), _ld(H), _vp(self.Z), _ld(self.Z), f,
                                       dt, *params, _vp(self._ws), self._ws_bytes,
                                       C.byref(self._p))
        _lib.check(fn_name, rc)

    def __call__(self) -> torch.Tensor:
        with torch.cuda.device(self.graph.device):
            rc = _lib.load().appnp_plan_launch(self._p, _stream(self.graph.device))
        _lib.check("appnp_plan_launch", rc)
        return self.Z

    def close(self):
        if getattr(self, "_p", None):
            _lib.load().appnp_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SolvePlan(PropagatePlan):
    """A captured exact solve (``appnp_plan_create_solve``): the Chebyshev steps of
    ``solve_forward`` recorded once into a hipGraph for fixed H / Z buffers.  Used like
    ``PropagatePlan``: refill ``plan.H`` in place, call ``plan()``, read ``plan.Z``."""

    def __init__(self, graph: Graph, H: torch.Tensor, alpha: float = 0.1, tol: float = 1e-6,
                 iters: int | None = None):
        _check_dense("H", H, graph, graph.n)  # before alpha and tol, as ever
        self.iters = solve_iterations(alpha, tol) if iters is None else int(iters)
        self._capture("appnp_plan_create_solve", graph, H, (self.iters, float(alpha)))


KERNEL_KINDS = {_lib.KT_COPY: "copy", _lib.KT_STEP: "step", _lib.KT_REM: "rem",
                _lib.KT_LOCAL: "local", _lib.KT_REMOTE: "remote", _lib.KT_XCHG: "xchg",
                _lib.KT_PUSH: "push"}


def kernel_times(fn, device, max_launches: int = 1024) -> list[tuple[str, float]]:
    """Call ``fn()`` with the library's per-launch timer on (``appnp_kernel_timer_begin`` /
    ``_end``) and return one (kind, ms) pair per launch it enqueued, in launch order: "copy"
    (the split copy), "step" (the SpMM kernel), "local" / "remote" (its two halves on a
    row-partitioned graph), "rem" (the remainder pass), "xchg" (an exchange of the library's
    own row loop), "push" (the forward-push launch of ``push_columns``).  Each interval is
    bracketed by events right before and after its launch on the launch stream, so no wait
    before it is counted; no profiler runs."""
    lib = _lib.load()
    with torch.cuda.device(device):
        # fn() runs even if the timer cannot start: at N > 1 it may hold collectives that every
        # rank must join
        rc0 = lib.appnp_kernel_timer_begin(int(max_launches), _stream(device))
        try:
            fn()
        finally:
            ms = (C.c_float * max_launches)()
            kinds = (C.c_int * max_launches)()
            n = C.c_int(0)
            rc = lib.appnp_kernel_timer_end(ms, kinds, max_launches, C.byref(n)) if rc0 == 0 else 0
        _lib.check("appnp_kernel_timer_begin", rc0)
        _lib.check("appnp_kernel_timer_end", rc)
    return [(KERNEL_KINDS.get(kinds[i], str(kinds[i])), float(ms[i]))
            for i in range(min(n.value, max_launches))]


def line_rate_probe(table: torch.Tensor, lines: int, seed: int = 0, reps: int = 3) -> dict:
    """The device's random 128-B line rate (``appnp_line_rate_probe``): ``lines`` random lines
    gathered from ``table``'s storage (read only) per launch, one warm-up launch, then the
    median of ``reps`` launches timed with HIP events on the current stream.  Returns
    {"G_lines_s", "ms", "lines", "table_MB"}."""
    if not table.is_cuda:
        raise ValueError("table must be a device tensor")
    lib = _lib.load()
    dev = table.device
    base = table.untyped_storage().data_ptr()
    nbytes = table.untyped_storage().nbytes()
    skip = (-base) % 128  # the kernel gathers whole 128-B lines from a 128-B aligned start
    tbytes = (nbytes - skip) // 128 * 128
    sink = torch.zeros(1, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    times = []
    with torch.cuda.device(dev):
        for r in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            _lib.check("appnp_line_rate_probe", lib.appnp_line_rate_probe(
                C.c_void_p(base + skip), tbytes, int(lines), int(seed + r) & (2**64 - 1),
                C.c_void_p(sink.data_ptr()), C.c_void_p(stream.cuda_stream)))
            b.record(stream)
            times.append((a, b))
        torch.cuda.synchronize(dev)
    ms = sorted(a.elapsed_time(b) for a, b in times[1:])[reps // 2]
    return {"G_lines_s": lines / (ms * 1e-3) / 1e9, "ms": ms, "lines": int(lines),
            "table_MB": tbytes / 2**20}
