"""The numpy reference of appnp_push_topk (include/ppnp_amd.h): the replayed
forward-push block of tests/push_ref.py, the scales applied in fp32 as two separately rounded
products, and per column a stable argsort of (-v, index) -- the total order of
tests/test_gpu_topk.py::reference -- cut at k and sorted by index.  A column with fewer than k
positive entries pads itself: its zeros tie, and a stable sort keeps them in index order.
"""

import numpy as np

import push_ref


def candidates(X, row_scale=None, col_scale=None):
    """v = (X * row_scale[:, None]) * col_scale[None, :] in fp32, a None scale not applied."""
    V = np.asarray(X, dtype=np.float32)
    if row_scale is not None:
        V = V * np.asarray(row_scale, dtype=np.float32)[:, None]
    if col_scale is not None:
        V = V * np.asarray(col_scale, dtype=np.float32)[None, :]
    assert V.dtype == np.float32
    return V


def select(V, k):
    """(idx int32 [b, k] ascending, val fp32 [b, k]) of the fp32 candidates V [n, b] >= 0."""
    n, b = V.shape
    assert 1 <= k <= n and not np.isnan(V).any() and (V >= 0).all()
    idx = np.empty((b, k), dtype=np.int32)
    for c in range(b):
        order = np.argsort(-V[:, c].astype(np.float64), kind="stable")[:k]
        idx[c] = np.sort(order)
    val = np.ascontiguousarray(V.T)[np.arange(b)[:, None], idx]
    return idx, val


def push_topk(indptr, indices, vals, sources, alpha, eps, k, w=None, max_rounds=1000,
              row_scale=None, col_scale=None):
    """(idx int32 [b, k], val fp32 [b, k], rounds int32 [b], left int32 [b], V fp32 [n, b]):
    V is the candidate block the rows were selected from."""
    X, rounds, left, _ = push_ref.push_columns(indptr, indices, vals, sources, alpha, eps, w,
                                               max_rounds)
    V = candidates(X, row_scale, col_scale)
    idx, val = select(V, k)
    return idx, val, rounds, left, V


def short_and_tied(V, k):
    """(columns with fewer than k positive candidates, columns whose k-th and (k+1)-th largest
    candidates are equal and positive: the tie rule decides what is kept)."""
    n, b = V.shape
    short = (V > 0).sum(axis=0) < k
    if k >= n:
        return short, np.zeros(b, dtype=bool)
    top = -np.sort(-V, axis=0)[:k + 1]
    return short, (top[k - 1] == top[k]) & (top[k] > 0)
