"""CPU: the ABI of the device minibatch slice (appnp_csr_batch_count / _emit) and its glue.

No compute call is made (there is no GPU here): the exports, the argument validation that returns
before touching the device, the workspace size, the ``slicer=`` / ``--batch-slice`` plumbing, and
the numpy reference the GPU tests compare with (tests/csr_batch_ref.py), pinned here to today's
torch ``SparsePPR.batch`` on CPU tensors.
"""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import csr_batch_ref as R
from test_topk_abi import DENSE


def _lib():
    from ppnp_amd import _lib

    return _lib, _lib.load()


NAMES = ("appnp_csr_batch_workspace_bytes", "appnp_csr_batch_count", "appnp_csr_batch_emit")


def test_csr_batch_symbols_exported():
    L, lib = _lib()
    for name in NAMES:
        assert name in L.EXPORTED
        assert hasattr(lib, name)
    assert lib.appnp_abi_version() == 2  # a backward-compatible addition
    from ppnp_amd import ops

    # the constants the GPU tests derive their shapes from are the header's
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "ppnp_amd.h")).read()
    assert f"#define APPNP_CSR_BATCH_SCAN_PASS {ops.CSR_BATCH_SCAN_PASS}\n" in header
    assert f"#define APPNP_CSR_BATCH_LDS_COLS {ops.CSR_BATCH_LDS_COLS}\n" in header


P_ = C.c_void_p(0x1000)  # never dereferenced on the host
BIG = 1 << 40


def _count(rows=100, cols=50, b=4, indptr=P_, idx=P_, out_indptr=P_, counts=P_, ws=P_,
           ws_bytes=BIG):
    _, lib = _lib()
    return lib.appnp_csr_batch_count(indptr, P_, P_, rows, cols, idx, b, out_indptr, counts, ws,
                                     ws_bytes, None)


def _emit(rows=100, cols=50, b=4, nnz_out=10, n_sel=5, indptr=P_, indices=P_, vals=P_, idx=P_,
          out_indptr=P_, oi=P_, ov=P_, sel=P_, tp=P_, ti=P_, tv=P_, ws=P_, ws_bytes=BIG):
    _, lib = _lib()
    return lib.appnp_csr_batch_emit(indptr, indices, vals, rows, cols, idx, b, out_indptr,
                                    nnz_out, n_sel, oi, ov, sel, tp, ti, tv, ws, ws_bytes, None)


def test_count_argument_validation_without_device():
    """Every APPNP_EINVAL case of include/ppnp_amd.h returns before any device call."""
    L, lib = _lib()
    E, OK = L.APPNP_EINVAL, L.APPNP_OK
    assert _count(rows=-1) == E
    assert _count(cols=-1) == E
    assert _count(b=-1) == E
    assert _count(cols=2**31) == E
    assert _count(b=2**31) == E
    for name in ("indptr", "idx", "out_indptr", "counts", "ws"):
        assert _count(**{name: None}) == E, name
    need = lib.appnp_csr_batch_workspace_bytes(50, 4, 0)
    assert need > 0
    assert _count(ws_bytes=need - 1) == E
    assert _count(ws_bytes=0) == E
    assert _count(ws=C.c_void_p(0x1004)) == E  # not 8-byte aligned
    # empty shapes: nothing to do, whatever the pointers are
    assert _count(b=0) == OK
    assert _count(cols=0) == OK
    assert _count(b=0, indptr=None, idx=None, out_indptr=None, counts=None, ws=None,
                  ws_bytes=0) == OK
    # ... but a bad shape argument is still refused on an empty shape
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
    assert _emit(n_sel=-1) == E
    assert _emit(nnz_out=2**31, n_sel=5) == E
    assert _emit(n_sel=51, nnz_out=60) == E   # more selected columns than columns
    assert _emit(n_sel=11, nnz_out=10) == E   # every selected column holds a kept entry
    for name in ("indptr", "idx", "out_indptr", "tp", "ws", "indices", "vals", "oi", "ov", "sel",
                 "ti", "tv"):
        assert _emit(**{name: None}) == E, name
    need = lib.appnp_csr_batch_workspace_bytes(50, 4, 200)  # rounded to 256 bytes
    assert need > lib.appnp_csr_batch_workspace_bytes(50, 4, 0)
    assert _emit(nnz_out=200, ws_bytes=need - 1) == E
    count_bytes = lib.appnp_csr_batch_workspace_bytes(50, 4, 0)  # enough for count, not for emit
    assert _emit(nnz_out=200, ws_bytes=count_bytes) == E
    assert _emit(ws_bytes=0) == E
    assert _emit(ws=C.c_void_p(0x1004)) == E
    assert _emit(b=0) == OK
    assert _emit(cols=0, n_sel=0) == OK
    assert _emit(b=0, nnz_out=0, n_sel=0, indptr=None, indices=None, vals=None, idx=None,
                 out_indptr=None, oi=None, ov=None, sel=None, tp=None, ti=None, tv=None, ws=None,
                 ws_bytes=0) == OK
    assert _emit(b=0, nnz_out=-1) == E
    assert _emit(b=0, n_sel=-1) == E


def test_csr_batch_workspace_bytes_monotone_and_empty():
    _, lib = _lib()
    ws = lib.appnp_csr_batch_workspace_bytes
    assert ws(0, 128, 8) == 0 and ws(1000, 0, 8) == 0 and ws(0, 0, 0) == 0
    assert ws(-1, 4, 1) == 0 and ws(4, -1, 1) == 0 and ws(4, 4, -1) == 0
    cs = [1, 31, 32, 33, 64, 65, 2810, 169_343, 2_449_029, 2**31 - 1]
    bs = [1, 2, 127, 128, 1024, 4096, 4097, 100_000]
    zs = [0, 1, 63, 64, 16_384, 131_072, 10_000_000, 2**31 - 1]
    for b in bs:
        for z in zs:
            sizes = [ws(c, b, z) for c in cs]
            assert all(s > 0 for s in sizes)
            assert sizes == sorted(sizes), (b, z, sizes)
    for c in cs:
        for z in zs:
            sizes = [ws(c, b, z) for b in bs]
            assert sizes == sorted(sizes), (c, z, sizes)
        for b in bs:
            sizes = [ws(c, b, z) for z in zs]
            assert sizes == sorted(sizes), (c, b, sizes)
    # nothing N-sized beyond the bitmap and its word ranks: products-synth, b = 128, k = 128
    n, z = 2_449_029, 128 * 128
    assert ws(n, 128, z) <= 2 * 4 * ((n + 31) // 32) + 4 * 128 + 12 * z + 512


def test_slicer_argument():
    from ppnp_amd.ppr import SparsePPR

    P = SparsePPR.from_dense(torch.from_numpy(DENSE))
    idx = torch.tensor([0, 3])
    with pytest.raises(ValueError, match="slicer"):
        P.batch(idx, slicer="bogus")
    with pytest.raises(ValueError, match="GPU"):
        P.batch(idx, slicer="device")  # a CPU matrix: there is no fallback
    a, sa = P.batch(idx)
    b, sb = P.batch(idx, slicer="torch")  # the default
    assert torch.equal(sa, sb) and torch.equal(a.indices, b.indices)


def test_trainer_takes_batch_slice(capsys):
    from ppnp_amd import train

    base = ["--batch-size", "32", "--ppr-topk", "32"]
    assert train.parse_args(base + ["--batch-slice", "device"]).batch_slice == "device"
    assert train.parse_args(base + ["--batch-slice", "torch"]).batch_slice == "torch"
    assert train.parse_args(base).batch_slice == "torch"
    assert train.parse_args([]).batch_slice == "torch"
    with pytest.raises(SystemExit):
        train.parse_args(["--batch-slice", "device"])
    assert "--batch-slice" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--batch-slice", "host"])


# ---- the reference, pinned to the torch route on CPU tensors --------------------------------

def _torch_batch(case, idx):
    from ppnp_amd.ppr import SparsePPR

    indptr, indices, data, shape = case
    P = SparsePPR(indptr, indices, data, shape, device="cpu")
    sub, sel = P.batch(torch.as_tensor(np.asarray(idx, dtype=np.int64)))
    return sub, sel


def same_bits(a, b):
    """Equal as bit patterns (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_torch(case, idx):
    ref = R.csr_batch_ref(*case, idx)
    sub, sel = _torch_batch(case, idx)
    assert sub.shape == (len(idx), len(ref[3]))
    assert same_bits(sub.indptr.numpy(), ref[0])
    assert same_bits(sub.indices.numpy(), ref[1])
    assert same_bits(sub.data.numpy(), ref[2])
    assert sel.dtype == torch.int64 and same_bits(sel.numpy(), ref[3])
    # the literal dense protocol for the selection: d = dense[idx]; mask = (d > 0).any(0)
    indptr, indices, data, shape = case
    dense = np.zeros(shape, dtype=np.float32)
    dense[np.repeat(np.arange(shape[0]), np.diff(indptr)), indices] = data
    with np.errstate(invalid="ignore"):
        mask = (dense[np.asarray(idx, dtype=np.int64)].reshape(len(idx), shape[1]) > 0).any(axis=0)
    assert ref[3].tolist() == np.flatnonzero(mask).tolist()
    return ref


def _dense_case():
    from ppnp_amd.ppr import SparsePPR

    P = SparsePPR.from_dense(torch.from_numpy(DENSE))
    return P.indptr.numpy(), P.indices.numpy(), P.data.numpy(), P.shape


@pytest.mark.parametrize("idx", [[0], [3, 0], [1], [4, 2, 2, 1], [0, 1, 2, 3, 4], []])
def test_reference_matches_torch_on_the_hand_written_matrix(idx):
    ref = check_against_torch(_dense_case(), idx)
    # ... and the dense protocol itself
    d = DENSE[idx].reshape(len(idx), 6)
    mask = (d > 0).any(axis=0)
    assert ref[3].tolist() == np.flatnonzero(mask).tolist()
    sub = np.zeros((len(idx), int(mask.sum())), dtype=np.float32)
    rows = np.repeat(np.arange(len(idx)), np.diff(ref[0]))
    sub[rows, ref[1]] = ref[2]
    assert np.array_equal(sub, d[:, mask])


def test_reference_on_the_non_positive_entries_of_test_topk_abi():
    ref = check_against_torch(([0, 2, 3], [1, 4, 4], [0.5, 0.0, -1.0], (2, 6)), [0, 1])
    assert ref[3].tolist() == [1] and ref[0].tolist() == [0, 1, 1] and ref[2].tolist() == [0.5]
    assert ref[4][0].tolist() == [0, 1] and ref[4][1].tolist() == [0]


@pytest.mark.parametrize("idx", [[0, 1, 2, 3, 4, 5], [1, 2, 3], [3], [3, 3], [5, 4, 0, 0, 2],
                                 [4], [1, 3, 5], []])
def test_reference_matches_torch_on_the_values_case(idx):
    ref = check_against_torch(R.values_case(), idx)
    if idx == [0, 1, 2, 3, 4, 5]:
        assert ref[3].tolist() == [0, 1, 2, 4, 6, 7]   # 3 and 5 hold no positive entry
        assert np.diff(ref[0]).tolist() == [3, 2, 3, 0, 0, 2]  # row 3 loses everything
    if idx == [1, 2, 3]:
        assert ref[3].tolist() == [1, 6, 7]  # column 2: only 0.0 and -0.0 -> dropped
        assert np.diff(ref[0]).tolist() == [1, 2, 0]


@pytest.mark.parametrize("idx", [list(range(8)), [0, 6, 5, 0, 3, 6], [7, 5, 5, 1, 0, 2, 4, 3, 6],
                                 [2], [0]])
def test_reference_matches_torch_on_the_wave_case(idx):
    check_against_torch(R.wave_case(), idx)


@pytest.mark.parametrize("cols", [1, 31, 32, 33, 63, 64, 65, 2049])
def test_reference_matches_torch_on_the_tail_cases(cols):
    case = R.tail_case(cols)
    for idx in ([0, 1, 2, 3], [3, 2, 0], [3], [1, 1]):
        ref = check_against_torch(case, idx)
        if 0 in idx and 1 in idx:
            assert ref[3][0] == 0 and ref[3][-1] == cols - 1


def test_reference_matches_torch_on_random_and_hub_cases():
    rng = np.random.default_rng(3)
    case = R.random_case(300, 500, (0, 40), seed=1)
    for b in (1, 2, 128):
        check_against_torch(case, rng.integers(0, 300, b))
    check_against_torch(case, rng.permutation(300))
    hub = R.hub_case(300)
    ref = check_against_torch(hub, rng.permutation(300))
    tp, ti, _ = ref[4]
    seg = np.diff(tp)
    assert seg.max() == 300 and (seg == 1).sum() == 600  # the hub and the one-entry columns


def test_reference_transpose_is_the_canonical_transpose():
    """scipy's CSR -> CSC conversion is the same stable transpose (no duplicates here)."""
    import scipy.sparse as sp

    case = R.random_case(60, 90, (0, 12), seed=8)
    idx = np.random.default_rng(4).integers(0, 60, 45)
    ip, ix, dv, sel, (tp, ti, tv) = R.csr_batch_ref(*case, idx)
    T = sp.csr_matrix((dv, ix, ip), shape=(45, len(sel))).tocsc()
    assert same_bits(T.indptr.astype(np.int32), tp)
    assert same_bits(T.indices.astype(np.int32), ti)
    assert same_bits(T.data, tv)
    # a column's rows ascend
    for c in range(len(sel)):
        assert (np.diff(ti[tp[c]:tp[c + 1]]) > 0).all()
