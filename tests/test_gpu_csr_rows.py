"""GPU: whole rows of a device CSR, ``ops.csr_rows`` (appnp_csr_rows_count / _emit) behind
``SparseFeatures.rows`` and ``SparsePPR.rows(idx, slicer="device")``.

Every case is compared on the raw bits (``np.array_equal`` with the values viewed as uint32) with
the numpy reference (tests/csr_rows_ref.py, pinned to scipy and to the torch route by
tests/test_csr_rows_abi.py), separately with ``SparsePPR.rows(slicer="torch")`` on the same device,
and its emitted transpose with ``appnp_csr_transpose`` of the slice (taken from a copy without the
emitted transpose).  There is no tolerance anywhere: the routes move the same fp32 values.

PASS is the number of items one pass of the single-workgroup scans covers
(``ops.CSR_BATCH_SCAN_PASS``): the count's scan takes a third pass at 2 PASS + 1 taken rows, the
scan of the transpose's row pointer at 2 PASS + 1 columns.  The sort of a transpose segment has
three paths: up to 64 entries (a wave), up to 1024 (one staged tile of the workgroup), longer.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import csr_batch_ref as B
import csr_rows_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from ppnp_amd import ops

    return ops


def make(case, cls=None):
    from ppnp_amd.ppr import SparsePPR

    indptr, indices, data, shape = case
    return (cls or SparsePPR)(indptr, indices, data, shape, device=DEV)


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and np.array_equal(a, b)


def csr_transpose_of(sub):
    """appnp_csr_transpose of the slice: a copy without the emitted transpose."""
    from ppnp_amd.sparse import SparseFeatures

    plain = SparseFeatures(sub.indptr, sub.indices, sub.data, sub.shape, device=sub.device)
    assert plain._t is None
    return plain.transpose()


def check(P, case, idx):
    """slicer="device" against the reference, against slicer="torch", its transpose against
    appnp_csr_transpose, and transpose=False against the same slice.  Returns the slice."""
    from ppnp_amd.ppr import SparsePPR

    idx = np.ascontiguousarray(idx, dtype=np.int64)
    tidx = torch.from_numpy(idx).to(DEV)
    sub = P.rows(tidx, slicer="device")
    ref = R.csr_rows_ref(*case, idx)
    assert type(sub) is SparsePPR and sub.shape == (len(idx), P.shape[1])
    assert sub.indptr.dtype == torch.int32 and sub.indices.dtype == torch.int32
    assert sub.data.dtype == torch.float32
    got = (sub.indptr, sub.indices, sub.data)
    for name, g, r in zip(("indptr", "indices", "data"), got, ref[:3]):
        assert same(g, r), f"{name} differs from the reference"
    tsub = P.rows(tidx)  # the torch route on the same device
    assert tsub.shape == sub.shape and tsub._t is None
    for name, g, t in zip(("indptr", "indices", "data"), got,
                          (tsub.indptr, tsub.indices, tsub.data)):
        assert same(g, t), f"{name} differs from slicer='torch'"
    assert sub._t is not None, "the device route emits the transpose"
    want = csr_transpose_of(sub)
    for name, g, w, r in zip(("t_indptr", "t_indices", "t_data"), sub._t, want, ref[3]):
        assert g.dtype == w.dtype
        assert same(g, w), f"{name} differs from appnp_csr_transpose"
        assert same(g, r), f"{name} differs from the reference"
    ip, ix, dv, t = _ops().csr_rows(P, tidx, transpose=False)
    assert t is None
    for name, g, n in zip(("indptr", "indices", "data"), got, (ip, ix, dv)):
        assert same(g, n), f"{name} differs with transpose=False"
    return sub


@pytest.fixture(scope="module", params=[1, 33, 65, 2049])
def lengths(request):
    case = R.lengths_case(request.param)
    return case, make(case)


def test_row_lengths_and_values(lengths):
    """Row lengths 0 ... 129 (empty rows first, in the middle and last) over 1, 33, 65 and 2049
    columns; the values are 0.0, -0.0, negatives, NaNs, denormals and infinity as bit patterns.
    All rows, reversed, and nothing but empty rows."""
    case, P = lengths
    n = P.shape[0]
    sub = check(P, case, np.arange(n))
    assert same(sub.indptr, case[0]) and same(sub.data, case[2])  # all rows in order: M itself
    check(P, case, np.arange(n)[::-1])
    sub = check(P, case, [n - 1, 0, 70])
    assert sub.nnz == 0 and sub._t[0].tolist() == [0] * (P.shape[1] + 1)


@pytest.mark.parametrize("b", [0, 1, 2, 128])
def test_batch_sizes(lengths, b):
    case, P = lengths
    idx = np.random.default_rng(30 + b).integers(0, P.shape[0], b)  # unsorted, with duplicates
    sub = check(P, case, idx)
    if b == 0:
        assert sub.shape == (0, P.shape[1]) and sub.indptr.tolist() == [0]
        assert sub._t[0].tolist() == [0] * (P.shape[1] + 1) and sub._t[1].numel() == 0


def test_a_matrix_without_entries():
    """indices / vals are NULL in the library call (an empty tensor's pointer is passed as NULL)."""
    case = B.csr_of([[], [], []], 40)
    P = make(case)
    assert P.indices.numel() == 0
    sub = check(P, case, [2, 0, 0, 1])
    assert sub.nnz == 0


def test_count_scan_passes():
    """2 PASS + 1 taken rows of 0 ... 3 entries: the count's scan makes three passes."""
    PASS = _ops().CSR_BATCH_SCAN_PASS
    b = 2 * PASS + 1
    case = B.random_case(b, 700, (0, 3), seed=12)
    P = make(case)
    check(P, case, np.random.default_rng(13).permutation(b))
    check(P, case, np.arange(PASS + 1))


def test_transpose_scan_passes():
    """2 PASS + 1 columns, none of them empty: three passes of the transpose's row-pointer scan,
    every item non-zero; the entries of a row are not sorted."""
    cols = 2 * _ops().CSR_BATCH_SCAN_PASS + 1
    case = R.dense_columns_case(cols)
    sub = check(make(case), case, [2, 0, 1])
    assert (np.diff(sub._t[0].cpu().numpy()) == 1).all()
    check(make(case), case, [1, 1, 0, 2, 1])


@pytest.mark.parametrize("n", [64, 65, 300, 1100])
def test_hub_columns(n):
    """One row taken n times among others: each of its columns is a transpose segment of n (or
    n + 1) entries from the same source row -- the last wave-sorted length, the first staged one,
    one tile, more than one tile of 1024."""
    case = B.hub_case(40)
    idx = np.array([5] * n + [1, 2, 6, 39], dtype=np.int64)
    np.random.default_rng(n).shuffle(idx)
    sub = check(make(case), case, idx)
    seg = np.diff(sub._t[0].cpu().numpy())
    assert seg.max() == n + 4 and (seg == n).sum() == 2  # the hub; row 5's own two columns


def test_two_runs_are_identical():
    case = B.hub_case(40)
    P = make(case)
    idx = np.array([5] * 300 + list(range(40)), dtype=np.int64)
    np.random.default_rng(1).shuffle(idx)
    tidx = torch.from_numpy(idx).to(DEV)

    def run():
        sub = P.rows(tidx, slicer="device")
        return [t.cpu().numpy().tobytes() for t in (sub.indptr, sub.indices, sub.data) + sub._t]

    assert run() == run()


def test_out_of_range_indices(lengths):
    """IndexError from every wrapper; at the library level the count and the empty rows."""
    from ppnp_amd import _lib
    from ppnp_amd.sparse import SparseFeatures

    case, P = lengths
    rows, cols = P.shape
    X = make(case, SparseFeatures)
    for bad in ([3, rows, 7], [-1, 2], [5, rows, -1, 1]):
        t = torch.tensor(bad, device=DEV)
        with pytest.raises(IndexError):
            P.rows(t, slicer="device")
        with pytest.raises(IndexError):
            X.rows(t)
        with pytest.raises(IndexError):
            _ops().csr_rows(P, t, transpose=False)
    lib = _lib.load()
    idx = torch.tensor([129, rows, -1, 3, 2**40, 128], device=DEV)
    b = idx.numel()
    vp = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
    ip = torch.empty(b + 1, dtype=torch.int32, device=DEV)
    counts = torch.empty(2, dtype=torch.int64, device=DEV)
    src = (vp(P.indptr), vp(P.indices), vp(P.data), rows, cols, vp(idx), b)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    assert lib.appnp_csr_rows_count(*src, vp(ip), vp(counts), stream) == 0
    lens = np.diff(case[0])
    want = [int(lens[129]), 0, 0, int(lens[3]), 0, int(lens[128])]
    assert counts.tolist() == [sum(want), 3]
    assert np.diff(ip.cpu().numpy()).tolist() == want
    nnz = sum(want)
    oi = torch.full((nnz,), -7, dtype=torch.int32, device=DEV)
    ov = torch.zeros(nnz, dtype=torch.float32, device=DEV)
    tp = torch.empty(cols + 1, dtype=torch.int32, device=DEV)
    ti = torch.empty(nnz, dtype=torch.int32, device=DEV)
    tv = torch.empty(nnz, dtype=torch.float32, device=DEV)
    need = lib.appnp_csr_rows_workspace_bytes(cols, nnz)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.appnp_csr_rows_emit(*src, vp(ip), nnz, vp(oi), vp(ov), vp(tp), vp(ti), vp(tv),
                                   vp(ws), need, stream) == 0
    ref = R.csr_rows_ref(*case, [129, 3, 128])  # the rows in range, at positions 0, 3 and 5
    assert same(oi, ref[1]) and same(ov, ref[2])
    assert same(tp, ref[3][0]) and same(tv, ref[3][2])
    assert same(ti, np.array([0, 3, 5], dtype=np.int32)[ref[3][1]])
    check(P, case, [5, rows - 1, 0, 1])  # a valid call on the same stream afterwards


# ---- Cora-ML: the matrices the trainer slices -----------------------------------------------

@pytest.fixture(scope="module")
def cora_parts(cora):
    """The L1-normalised attribute matrix (scipy, device CSR, dense), the sparsified PPR matrix
    (sym, k = 128) and the ``sel`` of one real b = 128 minibatch: built once."""
    import ppnp_amd
    from ppnp_amd import train
    from ppnp_amd.ppr import sparsified_ppr
    from ppnp_amd.sparse import SparseFeatures

    n = int(cora["n"])
    adj = sp.csr_matrix((cora["adj_data"], cora["adj_indices"], cora["adj_indptr"]), shape=(n, n))
    attr = sp.csr_matrix((cora["attr_data"], cora["attr_indices"], cora["attr_indptr"]),
                         shape=tuple(cora["attr_shape"]))
    Xsp = sp.csr_matrix(train.normalize_attributes(attr), dtype=np.float32)
    Xsp.sort_indices()
    Xs = SparseFeatures.from_scipy(Xsp, device=DEV)
    G = ppnp_amd.Graph.from_scipy(adj, mode="sym", device=DEV)
    P = sparsified_ppr(G, 128, tol=1e-6)
    idx = torch.from_numpy(np.random.default_rng(5).permutation(n)[:128]).to(DEV)
    sub, sel = P.batch(idx, slicer="device")
    return {"adj": adj, "Xsp": Xsp, "Xs": Xs, "P": P, "idx": idx, "sub": sub, "sel": sel,
            "n_classes": int(cora["labels"].max()) + 1}


def test_cora_attribute_rows_of_a_real_batch(cora_parts):
    from ppnp_amd.sparse import SparseFeatures

    Xsp, Xs, sel = cora_parts["Xsp"], cora_parts["Xs"], cora_parts["sel"]
    assert 128 < sel.numel() < Xs.shape[0]
    case = (Xsp.indptr, Xsp.indices, Xsp.data, Xsp.shape)
    check(make(case), case, sel.cpu().numpy())
    sub = Xs.rows(sel)
    assert type(sub) is SparseFeatures and sub.shape == (sel.numel(), Xs.shape[1])
    S = Xsp[sel.cpu().numpy()]
    assert same(sub.indptr, S.indptr.astype(np.int32)) and same(sub.data, S.data)
    assert same(sub.indices, S.indices.astype(np.int32))


def test_cora_ppr_rows_of_the_stopping_set(cora_parts):
    P = cora_parts["P"]
    case = tuple(t.cpu().numpy() for t in (P.indptr, P.indices, P.data)) + (P.shape,)
    check(P, case, np.random.default_rng(8).permutation(P.shape[0])[:500])


def _model(cora_parts, seed=3):
    import ppnp_amd

    torch.manual_seed(seed)
    return ppnp_amd.APPNP(cora_parts["Xs"].shape[1], cora_parts["n_classes"],
                          cora_parts["adj"]).to(DEV)


def test_model_step_equals_the_step_on_the_scipy_slice(cora_parts):
    """model(Xs.rows(sel), ppr=sub) in train mode (dropout 0.5, the same seed before each
    forward): logits and every parameter gradient equal those on from_scipy(X[sel]) -- the same
    CSR with its transpose from appnp_csr_transpose -- bit for bit."""
    from ppnp_amd.sparse import SparseFeatures

    Xsp, Xs, sub, sel = (cora_parts[k] for k in ("Xsp", "Xs", "sub", "sel"))
    model = _model(cora_parts).train()
    params = list(model.encoder.parameters())
    cot = torch.randn(128, cora_parts["n_classes"],
                      generator=torch.Generator().manual_seed(9)).to(DEV)

    def run(X):
        for p in params:
            p.grad = None
        torch.manual_seed(77)
        out = model(X, ppr=sub)
        (out * cot).sum().backward()
        return out.detach().clone(), [p.grad.detach().clone() for p in params]

    dev_rows = Xs.rows(sel)
    assert dev_rows._t is not None
    host_rows = SparseFeatures.from_scipy(Xsp[sel.cpu().numpy()], device=DEV)
    assert host_rows._t is None
    d_out, d_g = run(dev_rows)
    h_out, h_g = run(host_rows)
    assert host_rows._t is not None  # its backward built the transpose
    assert float(h_out.abs().max()) > 0
    assert torch.equal(d_out, h_out)
    for a, b in zip(d_g, h_g):
        assert float(b.abs().max()) > 0
        assert torch.equal(a, b)


def test_model_on_sparse_rows_matches_dense_rows(cora_parts):
    """Eval mode against model(Xd[sel], ppr=sub), at the tolerance of
    test_model_sparse_input_matches_dense."""
    Xsp, Xs, sub, sel = (cora_parts[k] for k in ("Xsp", "Xs", "sub", "sel"))
    Xd = torch.from_numpy(np.asarray(Xsp.todense())).to(DEV)
    model = _model(cora_parts).eval()
    with torch.no_grad():
        a = model(Xd[sel], ppr=sub)
        b = model(Xs.rows(sel), ppr=sub)
    assert float(a.abs().max()) > 0
    assert torch.allclose(a, b, atol=1e-5, rtol=1e-4)


def test_trainer_on_sparse_x_minibatches():
    """The dropout stream differs from the dense route's, so the band of
    test_cora_accuracy_sparse_input is asserted, not the digits."""
    from ppnp_amd import train as T

    s = T.main(["--dataset", "cora_ml", "--n-runs", "3", "--sparse-x", "--batch-size", "128",
                "--ppr-topk", "128", "--batch-slice", "device"])
    assert s["batch_slice"] == "device" and s["runs"] == 3
    assert 0.81 <= s["valid_acc_mean"] <= 0.89, s
