"""ppnp_amd -- MI355X (gfx950) APPNP propagation path for bkj/ppnp.

The hot path: A_hat construction (helpers.py:58-66) and the APPNP
propagation loop Z <- (1-a) A_hat Z + a H that replaces the dense PPR product of
model.py:63, as hand-written HIP kernels behind the C ABI in include/ppnp_amd.h.
"""

from . import _lib
from .graph import Graph
from .model import APPNP, GPRGNN, PPNP, CustomLinear
from .ops import (SolvePlan, heat_coefficients, poly, poly_backward, poly_forward,
                  ppr_coefficients, propagate, propagate_backward, propagate_forward, solve,
                  solve_backward, solve_forward, solve_iterations, split_copy, step, step_split,
                  topk_columns)
from .ppr import SparsePPR, sparsified_ppr, topk_rows
from .sparse import SparseFeatures, sparse_linear

__all__ = [
    "APPNP",
    "GPRGNN",
    "PPNP",
    "CustomLinear",
    "Graph",
    "propagate",
    "propagate_forward",
    "propagate_backward",
    "poly",
    "poly_forward",
    "poly_backward",
    "ppr_coefficients",
    "heat_coefficients",
    "solve",
    "solve_forward",
    "solve_backward",
    "solve_iterations",
    "SolvePlan",
    "step",
    "step_split",
    "split_copy",
    "SparseFeatures",
    "sparse_linear",
    "SparsePPR",
    "topk_columns",
    "topk_rows",
    "sparsified_ppr",
    "_lib",
]
