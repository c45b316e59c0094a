"""CPU: the ABI of the forward-push PPR columns (appnp_push_columns) and the algorithm itself.

No compute call is made (there is no GPU here): the exports, the argument validation that returns
before touching the device, the workspace size, and the numpy replay of the algorithm
(tests/push_ref.py, what the GPU tests compare the kernel with bit for bit) against the fp64
oracle's Pi on Cora-ML, with the bound of include/ppnp_amd.h: |Pi[j, s] - p_j| < eps w_j.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ppnp_oracle as O

import push_ref

ALPHA = 0.1


def _lib():
    from ppnp_amd import _lib

    return _lib, _lib.load()


def test_push_symbols_exported():
    L, lib = _lib()
    for name in ("appnp_push_workspace_bytes", "appnp_push_columns"):
        assert name in L.EXPORTED
        assert hasattr(lib, name)
    assert lib.appnp_abi_version() == L.ABI_VERSION == 2  # a backward-compatible addition
    from ppnp_amd import ops

    assert L.KT_PUSH == 7 and ops.KERNEL_KINDS[L.KT_PUSH] == "push"


class _GraphHead(C.Structure):
    """The leading fields of struct appnp_graph (ppnp_amd/csrc/appnp_internal.h), followed by
    zero bytes for the rest (every pointer NULL): a host-only stand-in that the validation reads
    and no device call ever sees."""
    _fields_ = [("n", C.c_int64), ("row_lo", C.c_int64), ("row_hi", C.c_int64),
                ("nnz_hat", C.c_int64), ("nnz_local", C.c_int64), ("nnz_remote", C.c_int64),
                ("mode", C.c_int), ("symmetric", C.c_int), ("rest", C.c_char * 2048)]


def _graph(n=100, row_lo=0, row_hi=None, mode=0, symmetric=1):
    return _GraphHead(n=n, row_lo=row_lo, row_hi=n if row_hi is None else row_hi, mode=mode,
                      symmetric=symmetric)


def test_push_argument_validation_without_device():
    """Every case of include/ppnp_amd.h returns its code before any device call."""
    L, lib = _lib()
    p = C.c_void_p(0x1000)  # never dereferenced on the host
    big = 1 << 50
    full = _graph()

    def call(g=full, b=4, alpha=0.1, eps=1e-4, max_rounds=10, ld_x=None, src=p, X=p, ws=p,
             ws_bytes=big):
        gp = None if g is None else C.cast(C.pointer(g), C.c_void_p)
        return lib.appnp_push_columns(gp, src, b, alpha, eps, max_rounds, X,
                                      b if ld_x is None else ld_x, None, None, ws, ws_bytes, None)

    E, OK, NS = L.APPNP_EINVAL, L.APPNP_OK, L.APPNP_ENOTSUP
    assert call(g=None) == E
    assert call(b=-1, ld_x=0) == E
    assert call(ld_x=3) == E                      # ld_x < b
    for alpha in (0.0, -0.1, 1.5, float("nan")):  # alpha outside (0, 1]
        assert call(alpha=alpha) == E
    for eps in (0.0, -1e-4, 1.0, 2.0, float("nan")):  # eps outside (0, 1)
        assert call(eps=eps) == E
    assert call(max_rounds=0) == E
    assert call(max_rounds=-3) == E
    # nothing to do, whatever the pointers are -- but only after the checks above
    assert call(b=0, ld_x=0, src=None, X=None, ws=None, ws_bytes=0) == OK
    assert call(g=_graph(n=0), src=None, X=None, ws=None, ws_bytes=0) == OK
    assert call(b=0, ld_x=0, eps=1.0) == E
    assert call(g=_graph(n=0), max_rounds=0) == E
    # a directed or partitioned graph with nothing to do is not an error either
    assert call(g=_graph(symmetric=0), b=0, ld_x=0) == OK
    assert call(src=None) == E
    assert call(X=None) == E
    assert call(ws=None) == E
    need = lib.appnp_push_workspace_bytes(100, 4)
    assert need > 0
    assert call(ws_bytes=need - 1) == E
    assert call(ws_bytes=0) == E
    # alpha = 1 is allowed; the sym graph passes every check up to here: only ws is too small
    assert call(alpha=1.0, ws_bytes=need - 1) == E
    # not supported: a directed graph, a row partition, rw without the transpose
    assert call(g=_graph(symmetric=0)) == NS
    assert call(g=_graph(row_lo=10)) == NS
    assert call(g=_graph(row_hi=50)) == NS
    assert call(g=_graph(mode=1)) == NS           # t_row_ptr is NULL
    assert call(g=_graph(mode=1, symmetric=0)) == NS


def test_push_workspace_bytes_monotone_and_empty():
    _, lib = _lib()
    ws = lib.appnp_push_workspace_bytes
    assert ws(0, 128) == 0 and ws(1000, 0) == 0 and ws(0, 0) == 0
    assert ws(-1, 4) == 0 and ws(4, -1) == 0
    ns = [1, 63, 64, 65, 1000, 70_001, 169_343, 2_449_029, 2**31 - 1]
    bs = [1, 3, 33, 128, 130, 1024]
    for b in bs:
        sizes = [ws(n, b) for n in ns]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes), (b, sizes)
    for n in ns:
        sizes = [ws(n, b) for b in bs]
        assert sizes == sorted(sizes), (n, sizes)
    # per source: r, p and the takes as int64 [n], two int32 lists of capacity n
    assert ws(1000, 8) >= 8 * 1000 * (3 * 8 + 2 * 4)


@pytest.fixture(scope="module")
def adj(cora):
    n = int(cora["n"])
    return sp.csr_matrix((cora["adj_data"], cora["adj_indices"], cora["adj_indptr"]), shape=(n, n))


@pytest.fixture(scope="module")
def sources(adj):
    deg = np.asarray(adj.sum(axis=1)).ravel()
    hub, low = int(deg.argmax()), int(deg.argmin())
    rest = np.setdiff1d(np.arange(adj.shape[0]), [hub, low])
    others = np.random.default_rng(5).choice(rest, 8, replace=False)
    return np.concatenate([[hub, low], others]).astype(np.int64)


@pytest.fixture(scope="module", params=["sym", "rw"])
def setup(request, adj, sources):
    """(mode, A_hat^T in fp32 as a CSR, threshold weights w, the oracle's Pi[:, sources])."""
    mode = request.param
    a_hat = O.calc_a_hat(adj, mode)
    at = sp.csr_matrix(a_hat.astype(np.float32).T)
    at.sort_indices()
    d = np.asarray(adj.sum(axis=1)).ravel().astype(np.float64) + 1.0
    w = np.sqrt(d) if mode == "sym" else np.ones_like(d)
    Pi = O.compute_ppr(adj, ALPHA, mode)[:, sources].copy()
    Pi.setflags(write=False)
    return mode, at, w, Pi


@pytest.mark.parametrize("eps", [1e-3, 1e-4])
def test_replay_meets_the_bound_against_the_oracle(setup, sources, eps):
    mode, at, w, Pi = setup
    thr = push_ref.thresholds(eps, at.shape[0], w if mode == "sym" else None)
    worst = 0.0
    for c, s in enumerate(sources):
        p, rounds, left, edges = push_ref.push_one(at.indptr, at.indices, at.data, thr, int(s),
                                                   ALPHA)
        ratio = float((np.abs(Pi[:, c] - p.astype(np.float64) / push_ref.SCALE) / w).max()) / eps
        print(f"{mode} eps {eps:g} source {s}: rounds {rounds}, edges {edges}, left {left}, "
              f"max |err| / (eps w) {ratio:.3f}")
        assert left == 0
        assert 0 < rounds < 1000
        worst = max(worst, ratio)
    assert worst < 1.0


def test_replay_edge_cases():
    # path 0 - 1 - 2, A_hat^T = A_hat (sym); the self loops make it 3 + 2 * 2 entries
    a = sp.csr_matrix(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=np.float32))
    at = sp.csr_matrix(O.calc_a_hat(a, "sym").astype(np.float32))
    thr = push_ref.thresholds(1e-4, 3)
    p, rounds, left, _ = push_ref.push_one(at.indptr, at.indices, at.data, thr, 7, ALPHA)
    assert (p == 0).all() and rounds == 0 and left == -1  # a source out of range
    p, rounds, left, edges = push_ref.push_one(at.indptr, at.indices, at.data, thr, 0, ALPHA,
                                               max_rounds=1)
    assert rounds == 1 and left > 0 and edges == 2
    X = push_ref.to_float(p)
    assert X[0] == np.float32(np.float64(np.float32(ALPHA))) and X[1] == 0 and X[2] == 0
    # the sum of p and r is the unit mass up to one truncation per addition
    X, rounds, left, edges = push_ref.push_columns(at.indptr, at.indices, at.data, [1, 1, 5],
                                                   ALPHA, 1e-4)
    assert np.array_equal(X[:, 0].view(np.uint32), X[:, 1].view(np.uint32))
    assert (X[:, 2] == 0).all() and list(left) == [0, 0, -1] and rounds[0] == rounds[1] > 0


def test_eps_and_tol_are_mutually_exclusive():
    from ppnp_amd import ppr

    class G:  # refused before the graph is touched
        symmetric = True
        device = "cpu"
        n = 3
        mode = "sym"

    for fn, args in ((ppr.ppr_columns, (G(), [0])), (ppr.topk_rows, (G(), [0], 2)),
                     (ppr.sparsified_ppr, (G(), 2))):
        with pytest.raises(ValueError, match="mutually exclusive"):
            fn(*args, tol=1e-6, eps=1e-4)


def test_trainer_takes_ppr_eps(capsys):
    from ppnp_amd import train

    a = train.parse_args(["--batch-size", "32", "--ppr-topk", "32", "--ppr-eps", "1e-4"])
    assert a.ppr_eps == 1e-4
    assert train.parse_args([]).ppr_eps is None
    with pytest.raises(SystemExit):
        train.parse_args(["--ppr-eps", "1e-4"])  # needs the minibatch protocol
    with pytest.raises(SystemExit):
        train.parse_args(["--batch-size", "32", "--ppr-topk", "32", "--ppr-eps", "2"])
