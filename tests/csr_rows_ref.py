"""numpy reference of taking whole rows of a CSR (``ops.csr_rows``, ``SparseFeatures.rows``,
``SparsePPR.rows``) with the transpose of the slice, and the cases that are not already in
tests/csr_batch_ref.py.

Taken row p is ``M[idx[p]]`` as stored: entries in their order, columns not relabelled, values
the same bits.  The transpose is the stable sort of the taken entries (which are in (p, position
in the row) order) by column: a column's entries ascend by batch position, then by position in
the row, as ``appnp_csr_transpose`` orders them.
"""

import numpy as np

from csr_batch_ref import csr_of


def csr_rows_ref(indptr, indices, data, shape, idx):
    """(indptr int32 [b + 1], indices int32, data fp32, (t_indptr int32 [cols + 1], t_indices
    int32, t_data fp32)) of the rows ``idx`` of the CSR."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    rows, cols = shape
    b = len(idx)
    assert ((idx >= 0) & (idx < rows)).all()
    lens = indptr[idx + 1] - indptr[idx]
    p = np.repeat(np.arange(b), lens)
    src = (np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in idx])
           if b else np.zeros(0)).astype(np.int64)
    col, val = indices[src], data[src]
    out_indptr = np.zeros(b + 1, dtype=np.int64)
    np.cumsum(lens, out=out_indptr[1:])
    order = np.argsort(col, kind="stable")
    t_indptr = np.zeros(cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=cols), out=t_indptr[1:])
    return (out_indptr.astype(np.int32), col.astype(np.int32), val,
            (t_indptr.astype(np.int32), p[order].astype(np.int32), val[order]))


def lengths_case(cols, seed=21):
    """Rows of every length 0 ... 129 (clipped to ``cols``) in that order, with an empty row put
    in after length 69 and another at the end: empty rows first, in the middle and last.
    The values cycle through 0.0, -0.0, negatives, NaN (two payloads), denormals and ordinary
    numbers, written as bit patterns."""
    rng = np.random.default_rng(seed)
    special = np.array([0x00000000, 0x80000000, 0xBF800000, 0x7FC00000, 0xFFC00001, 0x00000001,
                        0x807FFFFF, 0x3F000000, 0x7F800000], dtype=np.uint32).view(np.float32)
    rows = []
    for ln in list(range(70)) + [0] + list(range(70, 130)) + [0]:
        ln = min(ln, cols)
        c = np.sort(rng.choice(cols, ln, replace=False))
        rows.append((c, special[(np.arange(ln) + len(rows)) % len(special)]))
    indptr = np.zeros(len(rows) + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([len(c) for c, _ in rows])
    indices = np.concatenate([c for c, _ in rows]).astype(np.int32)
    data = np.concatenate([v for _, v in rows]).astype(np.float32)
    return indptr, indices, data, (len(rows), cols)


def dense_columns_case(cols, seed=23):
    """Three rows over ``cols`` columns whose union is every column (none empty), entries
    unsorted within a row."""
    rng = np.random.default_rng(seed)
    owner = rng.integers(0, 3, cols)
    rows = []
    for r in range(3):
        c = rng.permutation(np.flatnonzero(owner == r))
        rows.append([(int(j), float(j % 13) - 6.0) for j in c])
    return csr_of(rows, cols)
