"""numpy reference of the per-minibatch slice (``SparsePPR.batch`` / ``ops.csr_batch``) and the
hand-written cases both the CPU and the GPU tests use.

The reference follows the dense protocol of batch-main.py:140-142 -- ``d = dense[idx]``,
``mask = (d > 0).any(0)``, ``d[:, mask]`` -- with one piece of stored-entry bookkeeping beside it:
a stored entry <= 0 (or NaN) does not show in ``d > 0``, but it is kept when another taken row
selects its column, so the entries are carried as (row, column, value) triples and only the
selection follows the dense rule.  The transpose is the stable sort of the kept entries by their new
column: the rows of a column ascend by batch position, as ``appnp_csr_transpose`` orders them.
"""

import numpy as np


def csr_batch_ref(indptr, indices, data, shape, idx):
    """(indptr int32 [b + 1], indices int32, data fp32, sel int64, (t_indptr int32 [|sel| + 1],
    t_indices int32, t_data fp32)) of the rows ``idx`` of the CSR."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    rows, cols = shape
    b = len(idx)
    assert ((idx >= 0) & (idx < rows)).all()
    lens = indptr[idx + 1] - indptr[idx]
    p = np.repeat(np.arange(b), lens)  # batch position of every taken entry, in row order
    src = (np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in idx])
           if b else np.zeros(0)).astype(np.int64)
    col, val = indices[src], data[src]
    # the dense protocol: d = dense[idx]; mask = (d > 0).any(0).  Column j of d holds a value > 0
    # iff a taken entry in column j does, so the b x cols array itself is not formed (the scan
    # cases have 10^9 elements); tests/test_csr_batch_abi.py checks this against the literal
    # dense form on the small cases.
    with np.errstate(invalid="ignore"):
        pos = val > 0
    mask = np.zeros(cols, dtype=bool)
    mask[col[pos]] = True
    sel = np.flatnonzero(mask).astype(np.int64)
    new_of = np.cumsum(mask) - 1  # rank of a selected column in sel
    keep = mask[col]
    p, col, val = p[keep], new_of[col[keep]], val[keep]
    out_indptr = np.zeros(b + 1, dtype=np.int64)
    np.cumsum(np.bincount(p, minlength=b), out=out_indptr[1:])
    order = np.argsort(col, kind="stable")  # entries are in (p, position) order already
    t_indptr = np.zeros(len(sel) + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=len(sel)), out=t_indptr[1:])
    return (out_indptr.astype(np.int32), col.astype(np.int32), val, sel,
            (t_indptr.astype(np.int32), p[order].astype(np.int32), val[order]))


def csr_of(rows_of_entries, cols):
    """CSR arrays of a matrix given as one list of (column, value) pairs per row, in that
    order."""
    indptr = np.zeros(len(rows_of_entries) + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows_of_entries])
    flat = [e for r in rows_of_entries for e in r]
    indices = np.array([c for c, _ in flat], dtype=np.int32)
    data = np.array([v for _, v in flat], dtype=np.float32)
    return indptr, indices, data, (len(rows_of_entries), cols)


def values_case():
    """A 6 x 8 matrix of every kind of value.  Column 2: a 0.0 (row 1) and a -0.0 (row 2) beside
    row 0's positive entry (kept when row 0 is taken).  Column 5: only a negative and a NaN
    (never selected: both dropped, rows 1 and 3 get shorter).  Row 3 holds nothing but entries
    that are dropped: it loses all of them.  Row 4 is empty.  Column 7: NaN beside a positive."""
    nan = float("nan")
    rows = [[(0, 0.5), (2, 0.25), (7, nan)],
            [(2, 0.0), (5, -1.0), (6, 2.0)],
            [(1, 1.5), (2, -0.0), (7, 0.125)],
            [(3, 0.0), (5, nan)],
            [],
            [(0, -2.0), (4, 3.0)]]
    return csr_of(rows, 8)


def wave_case(seed=5):
    """Row lengths 0, 1, 63, 64, 65, 129, 0, 2 over 200 columns: positive values, about one
    entry in eight negative (kept or dropped by what the other taken rows select)."""
    rng = np.random.default_rng(seed)
    cols = 200
    rows = []
    for ln in (0, 1, 63, 64, 65, 129, 0, 2):
        c = np.sort(rng.choice(cols, ln, replace=False))
        v = rng.random(ln).astype(np.float32) + 0.5
        v[rng.random(ln) < 0.125] *= -1.0
        rows.append(list(zip(c.tolist(), v.tolist())))
    return csr_of(rows, cols)


def tail_case(cols):
    """Four rows over ``cols`` columns with entries at column 0, at cols - 1 and at every word
    boundary of the bitmap that exists; row 2 is empty, row 3 repeats row 0's columns with
    non-positive values."""
    marks = sorted({c for c in (0, 1, 30, 31, 32, 33, 62, 63, 64, cols // 2, cols - 2, cols - 1)
                    if 0 <= c < cols})
    # column 0 is marks[0] and cols - 1 is marks[-1]: each is positive in row 0 or in row 1
    row0 = [(c, 1.0 + c) for c in marks[::2]]
    row1 = [(c, 0.5 + c) for c in marks[1::2]]
    row3 = [(c, 0.0 if i % 2 else -1.0) for i, (c, _) in enumerate(row0)]
    return csr_of([row0, row1, [], row3], cols)


def random_case(rows, cols, per_row, seed, neg=0.1):
    """Up to ``per_row`` (an int or a (lo, hi) range) distinct random columns per row (that many
    draws, repeats removed), sorted; a share ``neg`` of the values is negative."""
    rng = np.random.default_rng(seed)
    lo, hi = (per_row, per_row) if np.isscalar(per_row) else per_row
    drawn = [np.unique(rng.integers(0, cols, ln)) for ln in rng.integers(lo, hi + 1, rows)]
    indptr = np.zeros(rows + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([len(c) for c in drawn])
    indices = np.concatenate(drawn + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = (rng.random(len(indices)) + 0.25).astype(np.float32)
    data[rng.random(len(indices)) < neg] *= -1.0
    return indptr, indices, data, (rows, cols)


def hub_case(b, cols=None, seed=11):
    """``b`` rows that all hold column 7 (the hub: a transpose segment of length b), each with
    two columns of its own beside it (segments of length 1) and every third row a negative entry
    in the shared column 3."""
    cols = 8 + 2 * b if cols is None else cols
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(b):
        ent = [(7, float(rng.random()) + 0.5), (8 + 2 * r, 1.0 + r), (9 + 2 * r, 2.0 + r)]
        if r % 3 == 0:
            ent.insert(0, (3, -1.0 - r))
        if r == 1:
            ent.insert(0, (3, 0.75))  # selects column 3: the negative entries there are kept
        rows.append(sorted(ent))
    return csr_of(rows, cols)
