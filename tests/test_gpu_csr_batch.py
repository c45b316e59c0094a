"""GPU: the device minibatch slice, ``SparsePPR.batch(idx, slicer="device")`` (ops.csr_batch,
appnp_csr_batch_count / _emit).

Every case is compared, bit for bit, with the numpy reference (tests/csr_batch_ref.py, pinned to
the torch route by tests/test_csr_batch_abi.py), separately with ``slicer="torch"`` on the same
device, and its emitted transpose with ``appnp_csr_transpose`` of the sub-matrix (taken from a copy
whose cached transpose is cleared).  There is no tolerance anywhere: the routes move the same
fp32 values.

The shapes are the smallest at which each kernel takes another path.  PASS is the number of items
one pass of the single-workgroup scans covers (``ops.CSR_BATCH_SCAN_PASS``, the header's
APPNP_CSR_BATCH_SCAN_PASS = 1024 threads x 4 items): the bitmap's rank scan takes a second pass
from PASS + 1 words, the row scan from PASS + 1 rows, the scan of the transpose's row pointer from
PASS + 1 selected columns.  The mark kernel gathers the bitmap in LDS up to
``ops.CSR_BATCH_LDS_COLS`` columns and marks it directly above.  The sort of a transpose segment
has three paths: up to 64 entries (a wave), up to 1024 (one staged tile of the workgroup), longer
(several tiles and chunks).
"""

import numpy as np
import pytest
import torch

import csr_batch_ref as R
from test_csr_batch_abi import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from ppnp_amd import ops

    return ops


def make(case):
    from ppnp_amd.ppr import SparsePPR

    indptr, indices, data, shape = case
    return SparsePPR(indptr, indices, data, shape, device=DEV)


def host(t):
    return t.cpu().numpy()


def csr_transpose_of(sub):
    """appnp_csr_transpose of the sub-matrix: a copy without the emitted transpose."""
    from ppnp_amd.ppr import SparsePPR

    plain = SparsePPR(sub.indptr, sub.indices, sub.data, sub.shape, device=sub.device)
    assert plain._t is None
    return plain.transpose()


def check(P, case, idx, ref=None):
    """slicer="device" against the reference, against slicer="torch", and its transpose against
    appnp_csr_transpose.  Returns the device sub-matrix and sel."""
    idx = np.asarray(idx, dtype=np.int64)
    tidx = torch.from_numpy(idx).to(DEV)
    sub, sel = P.batch(tidx, slicer="device")
    ref = R.csr_batch_ref(*case, idx) if ref is None else ref
    assert sub.shape == (len(idx), len(ref[3]))
    assert sub.indptr.dtype == torch.int32 and sub.indices.dtype == torch.int32
    assert sub.data.dtype == torch.float32 and sel.dtype == torch.int64
    got = (host(sub.indptr), host(sub.indices), host(sub.data), host(sel))
    for name, g, r in zip(("indptr", "indices", "data", "sel"), got, ref[:4]):
        assert same_bits(g, r), f"{name} differs from the reference"
    tsub, tsel = P.batch(tidx)  # the torch route on the same device
    assert tsub.shape == sub.shape
    for name, g, t in zip(("indptr", "indices", "data", "sel"), got,
                          (tsub.indptr, tsub.indices, tsub.data, tsel)):
        assert same_bits(g, host(t)), f"{name} differs from slicer='torch'"
    assert sub._t is not None, "the device route emits the transpose"
    want = csr_transpose_of(sub)
    for name, g, w, r in zip(("t_indptr", "t_indices", "t_data"), sub._t, want, ref[4]):
        assert g.dtype == w.dtype
        assert same_bits(host(g), host(w)), f"{name} differs from appnp_csr_transpose"
        assert same_bits(host(g), r), f"{name} differs from the reference"
    return sub, sel


@pytest.mark.parametrize("cols", [1, 31, 32, 33, 63, 64, 65, 2049])
def test_bitmap_tail(cols):
    case = R.tail_case(cols)
    P = make(case)
    sub, sel = check(P, case, [0, 1, 2, 3])
    assert int(sel[0]) == 0 and int(sel[-1]) == cols - 1
    check(P, case, [3, 2, 0])
    check(P, case, [3])  # nothing positive: no column selected, every entry dropped
    check(P, case, [1, 1])


@pytest.mark.parametrize("idx", [list(range(8)), [0, 6, 5, 0, 3, 6], [7, 5, 5, 1, 0, 2, 4, 3, 6],
                                 [2], [0], [0, 6]])
def test_wave_boundaries(idx):
    """Row lengths 0, 1, 63, 64, 65, 129; empty rows first, last and in the middle of idx."""
    case = R.wave_case()
    check(make(case), case, idx)


@pytest.mark.parametrize("idx", [[0, 1, 2, 3, 4, 5], [1, 2, 3], [3], [3, 3], [5, 4, 0, 0, 2],
                                 [4], [1, 3, 5]])
def test_values(idx):
    """0.0, -0.0, negative, NaN and positive entries: kept beside a selecting row, dropped (the row
    gets shorter, row 3 loses everything) without one."""
    case = R.values_case()
    sub, sel = check(make(case), case, idx)
    if idx == [0, 1, 2, 3, 4, 5]:
        assert sel.tolist() == [0, 1, 2, 4, 6, 7]
        assert np.diff(host(sub.indptr)).tolist() == [3, 2, 3, 0, 0, 2]


@pytest.fixture(scope="module")
def random_matrix():
    case = R.random_case(300, 500, (0, 40), seed=1)
    return case, make(case)


@pytest.mark.parametrize("b", [0, 1, 2, 128])
def test_batch_sizes(random_matrix, b):
    case, P = random_matrix
    idx = np.random.default_rng(30 + b).integers(0, 300, b)  # unsorted, with duplicates
    sub, sel = check(P, case, idx)
    if b == 0:
        assert sub.shape == (0, 0) and sub.indptr.tolist() == [0] and sel.numel() == 0
        assert sub._t[0].tolist() == [0]


def test_all_rows_taken(random_matrix):
    case, P = random_matrix
    check(P, case, np.random.default_rng(2).permutation(300))
    check(P, case, np.arange(300))


def test_a_matrix_without_entries():
    case = R.csr_of([[], [], []], 40)
    check(make(case), case, [2, 0, 0, 1])


def test_rank_scan_passes():
    """One bitmap word more than two passes of the rank scan cover, selected columns in the
    first and the last word and around the pass boundaries."""
    PASS = _ops().CSR_BATCH_SCAN_PASS
    cols = 32 * PASS * 2 + 5
    edge = [0, 31, 32 * PASS - 1, 32 * PASS, 32 * PASS + 1, 64 * PASS - 1, 64 * PASS, cols - 1]
    rng = np.random.default_rng(6)
    rows = []
    for r in range(40):
        c = np.unique(np.concatenate([rng.integers(0, cols, 30), edge[r % 8:r % 8 + 1]]))
        rows.append([(int(j), float(1 + (j % 7)) * (-1.0 if (j + r) % 5 == 0 else 1.0))
                     for j in c])
    case = R.csr_of(rows, cols)
    P = make(case)
    sub, sel = check(P, case, rng.permutation(40))
    assert int(sel[-1]) == cols - 1
    check(P, case, [8, 3])


@pytest.mark.parametrize("over", [0, 1])
def test_mark_paths(over):
    """The last column count whose bitmap the mark kernel gathers in LDS (``ops.
    CSR_BATCH_LDS_COLS``, the header's APPNP_CSR_BATCH_LDS_COLS) and the first that marks the
    global bitmap directly; 70 rows: three workgroups of the LDS path (4 waves x 8 rows), the
    last one partly filled."""
    cols = _ops().CSR_BATCH_LDS_COLS + over
    edge = [0, 31, 32, cols - 33, cols - 32, cols - 1]
    rng = np.random.default_rng(60 + over)
    rows = []
    for r in range(70):
        c = np.unique(np.concatenate([rng.integers(0, cols, r % 50), edge[r % 6:r % 6 + 1]]))
        rows.append([(int(j), float(1 + (j % 7)) * (-1.0 if (j + r) % 4 == 0 else 1.0))
                     for j in c])
    case = R.csr_of(rows, cols)
    P = make(case)
    sub, sel = check(P, case, rng.permutation(70))
    assert int(sel[0]) == 0 and int(sel[-1]) == cols - 1
    check(P, case, rng.integers(0, 70, 33))


def test_row_scan_and_transpose_scan_passes():
    """b = two passes of the row scan plus one, one or two entries per row; the selected columns
    (more than two passes of the transpose's scan, plus a few) are mostly one-entry segments."""
    PASS = _ops().CSR_BATCH_SCAN_PASS
    b = 2 * PASS + 1
    case = R.random_case(b, 40 * PASS + 3, (1, 2), seed=12, neg=0.05)
    P = make(case)
    sub, sel = check(P, case, np.random.default_rng(13).permutation(b))
    assert sel.numel() > 2 * PASS + 1
    sub, sel = check(P, case, np.arange(PASS + 1))


@pytest.mark.parametrize("b", [300, 1100])
def test_hub_column(b):
    """A column present in every taken row: a transpose segment longer than 64 and than 256
    (b = 300: one staged tile), and longer than 1024 (b = 1100: two tiles, two chunks), beside
    2 b columns with one entry each."""
    case = R.hub_case(b)
    P = make(case)
    idx = np.random.default_rng(b).permutation(b)
    sub, sel = check(P, case, idx)
    seg = np.diff(host(sub._t[0]))
    assert seg.max() == b and (seg == 1).sum() == 2 * b


def test_hub_is_reproducible():
    case = R.hub_case(300)
    P = make(case)
    tidx = torch.from_numpy(np.random.default_rng(300).permutation(300)).to(DEV)

    def run():
        sub, sel = P.batch(tidx, slicer="device")
        return [host(t).tobytes() for t in (sub.indptr, sub.indices, sub.data, sel) + sub._t]

    assert run() == run()


def test_out_of_range_indices_raise_and_leave_the_stream_usable(random_matrix):
    case, P = random_matrix
    rows = P.shape[0]
    for bad in ([3, rows, 7], [-1, 2], [5, rows, -1, 1]):
        with pytest.raises(IndexError):
            P.batch(torch.tensor(bad, device=DEV), slicer="device")
    check(P, case, [5, 299, 0, 1])  # a valid call on the same stream afterwards


# ---- Cora-ML: the matrices the trainer slices -----------------------------------------------

@pytest.fixture(scope="module")
def cora_adj(cora):
    import scipy.sparse as sp

    n = int(cora["n"])
    return sp.csr_matrix((cora["adj_data"], cora["adj_indices"], cora["adj_indptr"]), shape=(n, n))


@pytest.fixture(scope="module")
def cora_ppr(cora_adj):
    """sparsified_ppr(graph, 128, tol=1e-6) per mode, with its host arrays: built once."""
    import ppnp_amd
    from ppnp_amd.ppr import sparsified_ppr

    out = {}
    for mode in ("sym", "rw"):
        G = ppnp_amd.Graph.from_scipy(cora_adj, mode=mode, device=DEV)
        P = sparsified_ppr(G, 128, tol=1e-6)
        out[mode] = (P, (host(P.indptr), host(P.indices), host(P.data), P.shape))
    return out


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_cora_batches(cora_ppr, mode):
    P, case = cora_ppr[mode]
    perm = np.random.default_rng(41).permutation(P.shape[0])
    for i in range(4):
        check(P, case, perm[128 * i:128 * (i + 1)])


def test_cora_model_forward_and_backward_are_identical(cora, cora_adj, cora_ppr):
    """model(X[sel], ppr=sub), forward and backward, with sub from either slicer: the same CSR
    and the same transpose feed the same kernels, so logits and gradients are equal bit for bit."""
    import ppnp_amd

    P, _ = cora_ppr["sym"]
    n = int(cora["n"])
    gen = torch.Generator().manual_seed(9)
    X = torch.rand(n, 96, generator=gen).to(DEV)
    cot = torch.randn(128, 7, generator=gen).to(DEV)
    torch.manual_seed(3)
    model = ppnp_amd.APPNP(96, 7, cora_adj, drop_prob=0.0).to(DEV)
    model.train()
    params = list(model.encoder.parameters())
    idx = torch.from_numpy(np.random.default_rng(5).permutation(n)[:128]).to(DEV)

    def run(slicer):
        for p in params:
            p.grad = None
        sub, sel = P.batch(idx, slicer=slicer)
        had_t = sub._t is not None
        out = model(X[sel], ppr=sub)
        (out * cot).sum().backward()
        return had_t, out.detach().clone(), [p.grad.detach().clone() for p in params]

    t_had, t_out, t_g = run("torch")
    d_had, d_out, d_g = run("device")
    assert d_had and not t_had  # only the device route arrives with its transpose
    assert float(t_out.abs().max()) > 0
    assert torch.equal(d_out, t_out)
    for a, b in zip(d_g, t_g):
        assert float(b.abs().max()) > 0
        assert torch.equal(a, b)


def test_trainer_takes_the_device_slicer():
    from ppnp_amd import train

    common = ["--dataset", "cora_ml", "--n-runs", "1", "--max-epochs", "3", "--batch-size", "32",
              "--ppr-topk", "32"]
    a = train.main(common)
    b = train.main(common + ["--batch-slice", "device"])
    assert a["batch_slice"] == "torch" and b["batch_slice"] == "device"
    for ra, rb in zip(a["records"], b["records"]):  # the same bits: the same run
        assert ra["epoch"] == rb["epoch"]
        assert ra["stop_acc"] == rb["stop_acc"] and ra["valid_acc"] == rb["valid_acc"]
