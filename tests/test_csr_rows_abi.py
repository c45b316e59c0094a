"""CPU: the ABI of taking rows of a device CSR (appnp_csr_rows_count / _emit) and its glue.

No compute call is made (there is no GPU here): the exports, the argument validation that returns
before touching the device, the workspace size, the ``rows`` / ``slicer=`` / ``--sparse-x
--batch-slice device`` plumbing, and the numpy reference the GPU tests compare with
(tests/csr_rows_ref.py), pinned here to scipy and to today's torch ``SparsePPR.rows`` on CPU
tensors.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import csr_batch_ref as B
import csr_rows_ref as R
from test_csr_batch_abi import same_bits
from test_topk_abi import DENSE


def _lib():
    from ppnp_amd import _lib

    return _lib, _lib.load()


NAMES = ("appnp_csr_rows_workspace_bytes", "appnp_csr_rows_count", "appnp_csr_rows_emit")


def test_csr_rows_symbols_exported():
    L, lib = _lib()
    for name in NAMES:
        assert name in L.EXPORTED
        assert hasattr(lib, name)
    assert lib.appnp_abi_version() == 2  # a backward-compatible addition


P_ = C.c_void_p(0x1000)  # never dereferenced on the host
BIG = 1 << 40


def _count(rows=100, cols=50, b=4, indptr=P_, indices=P_, vals=P_, idx=P_, out_indptr=P_,
           counts=P_):
    _, lib = _lib()
    return lib.appnp_csr_rows_count(indptr, indices, vals, rows, cols, idx, b, out_indptr, counts,
                                    None)


def _emit(rows=100, cols=50, b=4, nnz_out=10, indptr=P_, indices=P_, vals=P_, idx=P_,
          out_indptr=P_, oi=P_, ov=P_, tp=P_, ti=P_, tv=P_, ws=P_, ws_bytes=BIG):
    _, lib = _lib()
    return lib.appnp_csr_rows_emit(indptr, indices, vals, rows, cols, idx, b, out_indptr, nnz_out,
                                   oi, ov, tp, ti, tv, ws, ws_bytes, None)


def test_count_argument_validation_without_device():
    """Every APPNP_EINVAL case of include/ppnp_amd.h returns before any device call."""
    L, _ = _lib()
    E, OK = L.APPNP_EINVAL, L.APPNP_OK
    assert _count(rows=-1) == E
    assert _count(cols=-1) == E
    assert _count(b=-1) == E
    assert _count(cols=2**31) == E
    assert _count(b=2**31) == E
    for name in ("indptr", "idx", "out_indptr", "counts"):
        assert _count(**{name: None}) == E, name
    # nothing taken: nothing to do, whatever the pointers are
    assert _count(b=0) == OK
    assert _count(b=0, indptr=None, indices=None, vals=None, idx=None, out_indptr=None,
                  counts=None) == OK
    # ... but a bad shape argument is still refused
    assert _count(b=0, rows=-1) == E
    assert _count(b=0, cols=-3) == E


def test_emit_argument_validation_without_device():
    L, lib = _lib()
    E, OK = L.APPNP_EINVAL, L.APPNP_OK
    assert _emit(rows=-1) == E
    assert _emit(cols=-1) == E
    assert _emit(b=-1) == E
    assert _emit(cols=2**31) == E
    assert _emit(b=2**31) == E
    assert _emit(nnz_out=-1) == E
    assert _emit(nnz_out=2**31) == E
    for name in ("indptr", "idx", "out_indptr", "indices", "vals", "oi", "ov", "ti", "tv", "ws"):
        assert _emit(**{name: None}) == E, name
    # without the transpose its arrays and the workspace are not used, the rest still is checked
    for name in ("indptr", "idx", "out_indptr", "indices", "vals", "oi", "ov"):
        assert _emit(tp=None, ti=None, tv=None, ws=None, ws_bytes=0, **{name: None}) == E, name
    need = lib.appnp_csr_rows_workspace_bytes(50, 200)  # rounded to 256 bytes
    assert need >= 4 * (50 + 2 * 200) and need % 256 == 0
    assert _emit(nnz_out=200, ws_bytes=need - 1) == E
    assert _emit(ws_bytes=0) == E
    assert _emit(ws=C.c_void_p(0x1002)) == E  # not 4-byte aligned
    assert _emit(b=0) == OK
    assert _emit(b=0, nnz_out=0, indptr=None, indices=None, vals=None, idx=None, out_indptr=None,
                 oi=None, ov=None, tp=None, ti=None, tv=None, ws=None, ws_bytes=0) == OK
    assert _emit(b=0, nnz_out=-1) == E
    assert _emit(b=0, rows=-1) == E


def test_csr_rows_workspace_bytes_monotone_and_empty():
    _, lib = _lib()
    ws = lib.appnp_csr_rows_workspace_bytes
    assert ws(0, 8) == 0 and ws(1000, 0) == 0 and ws(0, 0) == 0
    assert ws(-1, 4) == 0 and ws(4, -1) == 0
    cs = [1, 31, 32, 33, 64, 65, 2810, 8192, 169_343, 2_449_029, 2**31 - 1]
    zs = [1, 63, 64, 16_384, 131_072, 10_000_000, 2**31 - 1]
    for z in zs:
        sizes = [ws(c, z) for c in cs]
        assert all(s >= 4 * (c + 2 * z) for s, c in zip(sizes, cs))  # cursors and the pairs
        assert sizes == sorted(sizes), (z, sizes)
    for c in cs:
        sizes = [ws(c, z) for z in [0] + zs]
        assert sizes == sorted(sizes), (c, sizes)
    assert ws(2810, 128 * 128) <= 4 * (2810 + 2 * 128 * 128) + 256  # nothing else in it


def test_rows_need_a_gpu_matrix_and_a_known_slicer():
    from ppnp_amd import ops
    from ppnp_amd.ppr import SparsePPR
    from ppnp_amd.sparse import SparseFeatures

    P = SparsePPR.from_dense(torch.from_numpy(DENSE))
    idx = torch.tensor([0, 3])
    with pytest.raises(ValueError, match="slicer"):
        P.rows(idx, slicer="bogus")
    with pytest.raises(ValueError, match="GPU"):
        P.rows(idx, slicer="device")  # a CPU matrix: there is no fallback
    X = SparseFeatures(P.indptr, P.indices, P.data, P.shape, device="cpu")
    with pytest.raises(ValueError, match="GPU"):
        X.rows(idx)
    with pytest.raises(ValueError, match="GPU"):
        ops.csr_rows(X, idx)
    a, b = P.rows(idx), P.rows(idx, slicer="torch")  # the default
    assert torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices)
    assert torch.equal(a.data, b.data) and type(a) is SparsePPR


def test_trainer_takes_sparse_x_with_the_device_slice(capsys):
    from ppnp_amd import train

    base = ["--sparse-x", "--batch-size", "32", "--ppr-topk", "32"]
    a = train.parse_args(base + ["--batch-slice", "device"])
    assert a.sparse_x and a.batch_slice == "device" and a.batch_size == 32
    for extra in ([], ["--batch-slice", "torch"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + extra)
        err = capsys.readouterr().err
        assert "--sparse-x" in err
        assert "a minibatch takes the rows X[sel], which needs a dense X" in " ".join(err.split())


# ---- the reference, pinned to scipy and to the torch route on CPU tensors -------------------

def check_against_scipy_and_torch(case, idx):
    from ppnp_amd.ppr import SparsePPR

    indptr, indices, data, shape = case
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    ip, ix, dv, (tp, ti, tv) = R.csr_rows_ref(*case, idx)
    assert ip.dtype == np.int32 and ix.dtype == np.int32 and dv.dtype == np.float32
    sub = SparsePPR(indptr, indices, data, shape, device="cpu").rows(torch.from_numpy(idx))
    assert sub.shape == (len(idx), shape[1])
    assert same_bits(sub.indptr.numpy(), ip)
    assert same_bits(sub.indices.numpy(), ix)
    assert same_bits(sub.data.numpy(), dv)
    if len(idx) == 0:
        assert tp.tolist() == [0] * (shape[1] + 1) and len(ti) == 0
        return
    M = sp.csr_matrix((data, indices, indptr), shape=shape)
    S = M[idx]
    sorted_rows = all((np.diff(ix[ip[p]:ip[p + 1]]) > 0).all() for p in range(len(idx)))
    if sorted_rows:  # scipy keeps a row's entries as stored
        assert same_bits(S.indptr.astype(np.int32), ip)
        assert same_bits(S.indices.astype(np.int32), ix)
        assert same_bits(S.data, dv)
    T = S.T.tocsr()
    T.sort_indices()
    assert T.shape == (shape[1], len(idx))
    assert same_bits(T.indptr.astype(np.int32), tp)
    assert same_bits(T.indices.astype(np.int32), ti)
    assert same_bits(T.data, tv)
    for c in range(shape[1]):  # a column's batch positions ascend
        assert (np.diff(ti[tp[c]:tp[c + 1]]) > 0).all()


@pytest.mark.parametrize("idx", [[0], [3, 0], [4, 2, 2, 1], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0], []])
def test_reference_on_the_hand_written_matrix(idx):
    from ppnp_amd.ppr import SparsePPR

    P = SparsePPR.from_dense(torch.from_numpy(DENSE))
    case = (P.indptr.numpy(), P.indices.numpy(), P.data.numpy(), P.shape)
    check_against_scipy_and_torch(case, idx)
    ip, ix, dv, _ = R.csr_rows_ref(*case, idx)
    sub = np.zeros((len(idx), 6), dtype=np.float32)
    sub[np.repeat(np.arange(len(idx)), np.diff(ip)), ix] = dv
    assert np.array_equal(sub, DENSE[idx].reshape(len(idx), 6))


@pytest.mark.parametrize("cols", [1, 33, 65, 2049])
def test_reference_on_the_lengths_case(cols):
    case = R.lengths_case(cols)
    n = case[3][0]
    lens = np.diff(case[0])
    assert n == 132 and lens[0] == 0 and lens[70] == 0 and lens[-1] == 0
    assert lens.max() == min(129, cols)
    rng = np.random.default_rng(cols)
    check_against_scipy_and_torch(case, np.arange(n))
    check_against_scipy_and_torch(case, np.arange(n)[::-1])
    check_against_scipy_and_torch(case, rng.integers(0, n, 128))  # unsorted, with duplicates
    check_against_scipy_and_torch(case, [n - 1, 0, 70])  # nothing but empty rows


def test_reference_on_hub_and_unsorted_cases():
    check_against_scipy_and_torch(B.hub_case(40), [5] * 70 + [1, 2, 1])  # ties of one row
    check_against_scipy_and_torch(R.dense_columns_case(300), [2, 0, 1, 0])
    check_against_scipy_and_torch(B.csr_of([[], [], []], 40), [2, 0, 0, 1])
