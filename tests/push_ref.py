"""The numpy replay of appnp_push_columns (include/ppnp_amd.h): forward push in
int64 fixed point, units of 2^-44, synchronous rounds, with the kernel's exact expressions.
Every sum is an integer sum, so the replay reproduces the device's X, rounds and left bit for bit
whatever order the device adds in.

The matrix walked is A_hat^T as a CSR (``indptr``, ``indices``, fp32 ``vals``): row i holds the
entries (j, i) of column i of A_hat.  ``w``: the fp64 weights of the thresholds (1 / dinv for
'sym', None = all ones for 'rw').
"""

import numpy as np

ONE = np.int64(1) << np.int64(44)
SCALE = 2.0 ** 44


def thresholds(eps, n, w=None):
    """thr_j = max(1, ceil(eps * w_j * 2^44)) in fp64, eps the fp32 value."""
    w = np.ones(n, dtype=np.float64) if w is None else np.asarray(w, dtype=np.float64)
    t = np.ceil((np.float64(np.float32(eps)) * w) * SCALE)
    return np.maximum(t, 1.0).astype(np.int64)


def push_block(indptr, indices, vals, thr, sources, alpha, max_rounds=1000):
    """All ``sources`` in lockstep, each with its own state (row c of the [S, n] arrays, kept
    flat): (p int64 [S, n], rounds [S], left [S], edges visited [S]).  A source's rounds do not
    depend on the others: one that has finished simply has no frontier entries any more."""
    n = len(indptr) - 1
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    S = len(sources)
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    vals64 = np.asarray(vals, dtype=np.float32).astype(np.float64)
    a = np.float64(np.float32(alpha))
    beta = np.float64(np.float32(1.0) - np.float32(alpha))
    p = np.zeros(S * n, dtype=np.int64)
    r = np.zeros(S * n, dtype=np.int64)
    rounds = np.zeros(S, dtype=np.int64)
    edges = np.zeros(S, dtype=np.int64)
    valid = (sources >= 0) & (sources < n)
    start_at = np.arange(S, dtype=np.int64)[valid] * n + sources[valid]
    r[start_at] = ONE
    front = start_at[ONE >= thr[sources[valid]]]
    k = 0
    while len(front) and k < max_rounds:
        node = front % n
        base = front - node
        t = r[front].copy()
        r[front] = 0  # every take before every add
        p[front] += (t.astype(np.float64) * a).astype(np.int64)  # astype truncates
        start = indptr[node]
        lens = indptr[node + 1] - start
        tot = int(lens.sum())
        off = np.cumsum(lens) - lens
        pos = np.repeat(start - off, lens) + np.arange(tot, dtype=np.int64)
        add = ((np.repeat(t, lens).astype(np.float64) * vals64[pos]) * beta).astype(np.int64)
        cols = indices[pos] + np.repeat(base, lens)
        np.add.at(r, cols, add)
        src = base // n
        edges += np.bincount(src, weights=lens, minlength=S).astype(np.int64)
        rounds[np.unique(src)] += 1
        k += 1
        # F = { j : r_j >= thr_j }: a node that nothing was added to holds 0 (taken) or what it
        # held below its threshold before, so only the touched nodes can be in it
        touched = np.unique(cols)
        front = touched[r[touched] >= thr[touched % n]]
    left = np.bincount(front // n, minlength=S).astype(np.int64)
    left[~valid] = -1
    return p.reshape(S, n), rounds, left, edges


def push_one(indptr, indices, vals, thr, s, alpha, max_rounds=1000):
    """One source: (p int64 [n], rounds, left, edges visited)."""
    p, rounds, left, edges = push_block(indptr, indices, vals, thr, [s], alpha, max_rounds)
    return p[0], int(rounds[0]), int(left[0]), int(edges[0])


def to_float(p):
    """X = (float)((double)p * 2^-44)."""
    return (p.astype(np.float64) * (1.0 / SCALE)).astype(np.float32)


def push_columns(indptr, indices, vals, sources, alpha, eps, w=None, max_rounds=1000):
    """(X fp32 [n, b], rounds int32 [b], left int32 [b], edges int64 [b]); equal sources are
    replayed once."""
    n = len(indptr) - 1
    thr = thresholds(eps, n, w)
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    uniq, inv = np.unique(sources, return_inverse=True)
    p, rounds, left, edges = push_block(indptr, indices, vals, thr, uniq, alpha, max_rounds)
    X = np.ascontiguousarray(to_float(p).T[:, inv])
    return X, rounds[inv].astype(np.int32), left[inv].astype(np.int32), edges[inv]
