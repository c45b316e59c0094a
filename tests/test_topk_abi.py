"""CPU: the ABI of the column top-k selection (appnp_topk_columns) and the SparsePPR glue.

No compute call is made (there is no GPU here): only the exports, the argument validation that
returns before touching the device, the workspace size, and the torch-level row / batch slicing
of SparsePPR on CPU tensors.
"""

import ctypes as C

import numpy as np
import pytest
import torch


def _lib():
    from ppnp_amd import _lib

    return _lib, _lib.load()


def test_topk_symbols_exported():
    L, lib = _lib()
    for name in ("appnp_topk_workspace_bytes", "appnp_topk_columns"):
        assert name in L.EXPORTED
        assert hasattr(lib, name)
    assert lib.appnp_abi_version() == 2  # a backward-compatible addition


def test_topk_argument_validation_without_device():
    """Every APPNP_EINVAL case of include/ppnp_amd.h returns before any device call."""
    L, lib = _lib()
    p = C.c_void_p(0x1000)  # never dereferenced on the host
    big = 1 << 40

    def call(n=100, b=4, k=3, ld_x=None, ld_out=None, X=p, oi=p, ov=p, ws=p, ws_bytes=big):
        return lib.appnp_topk_columns(X, b if ld_x is None else ld_x, n, b, k, None, None, oi, ov,
                                      k if ld_out is None else ld_out, ws, ws_bytes, None)

    E = L.APPNP_EINVAL
    assert call(n=-1) == E
    assert call(b=-1, ld_x=0) == E
    assert call(ld_x=3) == E          # ld_x < b
    assert call(ld_out=2) == E        # ld_out < k
    assert call(k=0, ld_out=4) == E   # k < 1
    assert call(k=-5, ld_out=4) == E
    assert call(k=101, n=100) == E    # k > n with n * b > 0
    assert call(n=2**31) == E         # n > INT32_MAX
    assert call(X=None) == E
    assert call(oi=None) == E
    assert call(ov=None) == E
    assert call(ws=None) == E
    need = lib.appnp_topk_workspace_bytes(100, 4, 3)
    assert need > 0
    assert call(ws_bytes=need - 1) == E
    assert call(ws_bytes=0) == E
    # empty shapes: nothing to do, whatever k and the pointers are
    assert call(n=0, k=5) == L.APPNP_OK
    assert call(b=0, ld_x=0) == L.APPNP_OK
    assert call(n=0, X=None, oi=None, ov=None, ws=None, ws_bytes=0) == L.APPNP_OK
    # ... but a bad shape argument is still refused on an empty shape
    assert call(n=0, k=0) == E
    assert call(n=0, ld_x=1) == E


def test_topk_workspace_bytes_monotone_and_empty():
    _, lib = _lib()
    ws = lib.appnp_topk_workspace_bytes
    assert ws(0, 128, 8) == 0 and ws(1000, 0, 8) == 0 and ws(0, 0, 1) == 0
    assert ws(-1, 4, 1) == 0 and ws(4, -1, 1) == 0
    ns = [1, 63, 64, 65, 1000, 70_001, 169_343, 2_449_029, 2**31 - 1]
    bs = [1, 7, 31, 32, 33, 128, 130, 1024]
    for b in bs:
        sizes = [ws(n, b, 1) for n in ns]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes), (b, sizes)
    for n in ns:
        sizes = [ws(n, b, 1) for b in bs]
        assert sizes == sorted(sizes), (n, sizes)
    # a small share of the block it selects from: products-scale N x 128 fp32 is 1.25 GB
    assert ws(2_449_029, 128, 128) < 0.05 * 2_449_029 * 128 * 4


# a hand-written 5 x 6 matrix: row 1 is empty, column 4 is empty, row 3 holds an explicit entry
# that no batch row selects when it is the only one in its column
DENSE = np.array([[0.5, 0.0, 0.25, 0.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                  [0.0, 0.125, 0.0, 0.0, 0.0, 0.75],
                  [0.0, 0.0, 0.0, 1.0, 0.0, 0.5],
                  [0.25, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)


def _sp():
    from ppnp_amd.ppr import SparsePPR

    return SparsePPR.from_dense(torch.from_numpy(DENSE))


def test_sparse_ppr_from_dense_is_canonical_csr():
    P = _sp()
    assert P.shape == (5, 6) and P.nnz == 7
    assert P.indptr.dtype == torch.int32 and P.indices.dtype == torch.int32
    assert P.indptr.tolist() == [0, 2, 2, 4, 6, 7]
    assert P.indices.tolist() == [0, 2, 1, 5, 3, 5, 0]
    assert P.data.tolist() == [0.5, 0.25, 0.125, 0.75, 1.0, 0.5, 0.25]
    assert np.array_equal(P.to_dense().numpy(), DENSE)


@pytest.mark.parametrize("idx", [[0], [3, 0], [1], [4, 2, 2, 1], []])
def test_sparse_ppr_rows(idx):
    R = _sp().rows(torch.tensor(idx, dtype=torch.long))
    assert R.shape == (len(idx), 6)
    assert np.array_equal(R.to_dense().numpy(), DENSE[idx].reshape(len(idx), 6))


@pytest.mark.parametrize("idx", [[0], [3, 0], [1], [4, 2, 2, 1], [0, 1, 2, 3, 4], []])
def test_sparse_ppr_batch_matches_the_dense_protocol(idx):
    """batch-main.py:140-142 on the dense form: ppr_sub = ppr[idx]; sel = (ppr_sub > 0).any(0);
    ppr_sub[:, sel]."""
    sub, sel = _sp().batch(torch.tensor(idx, dtype=torch.long))
    d = torch.from_numpy(DENSE)[idx].reshape(len(idx), 6)
    mask = (d > 0).any(dim=0)
    assert sel.dtype == torch.int64
    assert sel.tolist() == mask.nonzero().flatten().tolist()
    assert sub.shape == (len(idx), int(mask.sum()))
    assert np.array_equal(sub.to_dense().numpy(), d[:, mask].numpy())


def test_sparse_ppr_batch_drops_stored_entries_that_are_not_positive():
    """A stored entry <= 0 does not select its column (the reference tests ``> 0``)."""
    from ppnp_amd.ppr import SparsePPR

    P = SparsePPR([0, 2, 3], [1, 4, 4], [0.5, 0.0, -1.0], (2, 6), device="cpu")
    sub, sel = P.batch(torch.tensor([0, 1]))
    assert sel.tolist() == [1]
    assert sub.shape == (2, 1)
    assert sub.indptr.tolist() == [0, 1, 1] and sub.indices.tolist() == [0]
    assert sub.data.tolist() == [0.5]


def test_trainer_refuses_sparse_x_with_batches(capsys):
    from ppnp_amd import train

    with pytest.raises(SystemExit):
        train.parse_args(["--batch-size", "32", "--ppr-topk", "32", "--sparse-x"])
    assert "--sparse-x" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(["--batch-size", "32"])  # no --ppr-topk
    a = train.parse_args([])
    assert a.batch_size is None and a.ppr_topk is None  # the full-batch path
