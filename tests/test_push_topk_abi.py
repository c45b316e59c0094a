"""CPU: the ABI of the top k straight from the forward push (appnp_push_topk).

No compute call is made (there is no GPU here): the exports, the argument validation that returns
before touching the device in the order include/ppnp_amd.h states, the workspace size, the Python
argument checks, and the numpy reference the GPU tests compare with (tests/push_topk_ref.py) on a
graph small enough to check by hand.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ppnp_oracle as O

import push_ref
import push_topk_ref

ALPHA = 0.1


def _lib():
    from ppnp_amd import _lib

    return _lib, _lib.load()


def test_push_topk_symbols_exported_and_bound():
    L, lib = _lib()
    for name in ("appnp_push_topk_workspace_bytes", "appnp_push_topk"):
        assert name in L.EXPORTED
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None  # bound with its signature
    assert lib.appnp_push_topk_workspace_bytes.restype is C.c_size_t
    assert len(lib.appnp_push_topk.argtypes) == 18
    assert lib.appnp_abi_version() == L.ABI_VERSION == 2  # a backward-compatible addition
    from ppnp_amd import ops

    assert callable(ops.push_topk) and ops.PUSH_TOPK_MAX_K == 1024


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


def test_push_topk_argument_validation_without_device():
    """Every case of include/ppnp_amd.h returns its code before any device call, in its order:
    EINVAL, then OK for an empty call, then the pointers and the workspace, then ENOTSUP."""
    L, lib = _lib()
    p = C.c_void_p(0x1000)  # never dereferenced on the host
    big = 1 << 50
    full = _graph()

    def call(g=full, b=4, alpha=0.1, eps=1e-4, max_rounds=10, k=8, ld_out=None, slots=2, src=p,
             oi=p, ov=p, ws=p, ws_bytes=big):
        gp = None if g is None else C.cast(C.pointer(g), C.c_void_p)
        return lib.appnp_push_topk(gp, src, b, alpha, eps, max_rounds, k, None, None, oi, ov,
                                   k if ld_out is None else ld_out, None, None, slots, ws,
                                   ws_bytes, None)

    E, OK, NS = L.APPNP_EINVAL, L.APPNP_OK, L.APPNP_ENOTSUP
    assert call(g=None) == E
    assert call(b=-1) == E
    assert call(ld_out=7) == E                    # ld_out < k
    for alpha in (0.0, -0.1, 1.5, float("nan")):  # alpha outside (0, 1]
        assert call(alpha=alpha) == E
    for eps in (0.0, -1e-4, 1.0, 2.0, float("nan")):  # eps outside (0, 1)
        assert call(eps=eps) == E
    assert call(max_rounds=0) == E
    assert call(max_rounds=-3) == E
    assert call(k=0, ld_out=4) == E
    assert call(k=-2, ld_out=4) == E
    assert call(slots=0) == E
    assert call(slots=-1) == E
    # nothing to do, whatever the pointers are -- but only after the checks above
    assert call(b=0, src=None, oi=None, ov=None, ws=None, ws_bytes=0) == OK
    assert call(g=_graph(n=0), src=None, oi=None, ov=None, ws=None, ws_bytes=0) == OK
    assert call(b=0, k=500) == OK                 # k > n is looked at after the empty call
    assert call(b=0, eps=1.0) == E
    assert call(b=0, slots=0) == E
    assert call(b=0, k=0, ld_out=0) == E
    assert call(g=_graph(n=0), max_rounds=0) == E
    # a directed or partitioned graph with nothing to do is not an error either
    assert call(g=_graph(symmetric=0), b=0) == OK
    assert call(k=101) == E                       # k > n
    assert call(src=None) == E
    assert call(oi=None) == E
    assert call(ov=None) == E
    assert call(ws=None) == E
    need = lib.appnp_push_topk_workspace_bytes(100, 2)
    assert need > 0
    assert call(ws_bytes=need - 1) == E
    assert call(ws_bytes=0) == E
    # the workspace is sized by `slots`, not by b
    assert call(slots=3, ws_bytes=need) == E
    assert call(alpha=1.0, ws_bytes=need - 1) == E
    # EINVAL comes before ENOTSUP: an unsupported graph with a short workspace
    assert call(g=_graph(symmetric=0), ws_bytes=need - 1) == E
    # not supported: a directed graph, a row partition, rw without the transpose
    assert call(g=_graph(symmetric=0)) == NS
    assert call(g=_graph(row_lo=10)) == NS
    assert call(g=_graph(row_hi=50)) == NS
    assert call(g=_graph(mode=1)) == NS           # t_row_ptr is NULL
    assert call(g=_graph(mode=1, symmetric=0)) == NS
    # k above the cap of the header, on a graph that passes every other check: refused before any
    # launch (k <= n is looked at first, so the graph must be large enough)
    from ppnp_amd import ops

    assert ops.PUSH_TOPK_MAX_K == 1024
    assert call(g=_graph(n=5000), k=1025) == NS
    assert call(g=_graph(n=1000), k=1025) == E    # k > n wins


def test_push_topk_workspace_bytes_monotone_empty_and_independent_of_b():
    _, lib = _lib()
    ws = lib.appnp_push_topk_workspace_bytes
    assert ws(0, 128) == 0 and ws(1000, 0) == 0 and ws(0, 0) == 0
    assert ws(-1, 4) == 0 and ws(4, -1) == 0
    assert ws(2**31, 1) == 0  # n beyond the int32 index range: no such call
    ns = [1, 63, 64, 65, 1000, 70_001, 169_343, 2_449_029, 2**31 - 1]
    slots = [1, 2, 3, 33, 128, 256, 1024]
    for s in slots:
        sizes = [ws(n, s) for n in ns]
        assert all(x > 0 for x in sizes)
        assert sizes == sorted(sizes), (s, sizes)
    for n in ns:
        sizes = [ws(n, s) for s in slots]
        assert sizes == sorted(sizes), (n, sizes)
    # per slot: r, p and the takes as int64 [n], two frontier lists and the taken list as int32;
    # the thresholds once
    assert ws(1000, 8) >= 8 * 1000 * (3 * 8 + 3 * 4) + 8 * 1000
    assert ws(1000, 8) < 8 * 1000 * 40 + 8 * 1000 + 4096
    # the signature has no b: all N sources of a graph run on the slots of one workspace
    assert len(lib.appnp_push_topk_workspace_bytes.argtypes) == 2


class _G:  # refused before the graph is touched
    symmetric = True
    device = "cpu"
    n = 3
    mode = "sym"
    row_lo = 0
    row_hi = 3


def test_select_lists_needs_eps_and_a_known_name():
    from ppnp_amd import ppr

    for fn, args in ((ppr.topk_rows, (_G(), [0], 2)), (ppr.sparsified_ppr, (_G(), 2))):
        with pytest.raises(ValueError, match="needs eps"):
            fn(*args, select="lists")
        with pytest.raises(ValueError, match="needs eps"):
            fn(*args, select="lists", tol=1e-6)
        with pytest.raises(ValueError, match="'block' or 'lists'"):
            fn(*args, select="rows", eps=1e-4)
        with pytest.raises(ValueError, match="mutually exclusive"):
            fn(*args, select="lists", tol=1e-6, eps=1e-4)


def test_push_topk_python_argument_checks():
    from ppnp_amd import ops

    class Directed(_G):
        symmetric = False

    class Part(_G):
        row_hi = 2

    with pytest.raises(ValueError, match="undirected"):
        ops.push_topk(Directed(), [0], 2)
    with pytest.raises(ValueError, match="row-partitioned"):
        ops.push_topk(Part(), [0], 2)
    for k in (0, -1, 4):  # outside [1, n]
        with pytest.raises(ValueError, match="k must be in"):
            ops.push_topk(_G(), [0], k)

    class Big(_G):
        n = 5000
        row_hi = 5000

    with pytest.raises(ValueError, match="at most k = 1024"):
        ops.push_topk(Big(), [0], 1025)
    with pytest.raises(ValueError, match="slots must be at least 1"):
        ops.push_topk(_G(), [0], 2, slots=0)


def test_sparse_ppr_cache_key_carries_select(monkeypatch):
    import inspect

    from ppnp_amd import ppr
    from ppnp_amd.model import APPNP

    assert inspect.signature(APPNP.sparse_ppr).parameters["select"].default == "block"
    built = []

    def fake(g, topk, K, alpha, tol=None, eps=None, info=None, select="block"):
        built.append(select)
        return (select, len(built))

    monkeypatch.setattr(ppr, "sparsified_ppr", fake)

    class Model:  # what sparse_ppr reads of the model
        alpha, PPR_TOL, _sparse_ppr = 0.1, APPNP.PPR_TOL, None

        def graph(self):
            return _G()

    m = Model()
    a = APPNP.sparse_ppr(m, 8, eps=1e-4)
    assert APPNP.sparse_ppr(m, 8, eps=1e-4, select="block") is a  # the default, cached
    b = APPNP.sparse_ppr(m, 8, eps=1e-4, select="lists")
    assert APPNP.sparse_ppr(m, 8, eps=1e-4, select="lists") is b
    assert built == ["block", "lists"] and a != b


def test_trainer_takes_ppr_select(capsys):
    from ppnp_amd import train

    base = ["--batch-size", "32", "--ppr-topk", "32"]
    a = train.parse_args(base + ["--ppr-eps", "1e-4", "--ppr-select", "lists"])
    assert a.ppr_select == "lists" and a.ppr_eps == 1e-4
    assert train.parse_args(base + ["--ppr-eps", "1e-4"]).ppr_select == "block"
    assert train.parse_args(base + ["--ppr-eps", "1e-4", "--ppr-select", "block"]).ppr_select \
        == "block"
    assert train.parse_args([]).ppr_select == "block"
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--ppr-select", "lists"])  # needs --ppr-eps
    with pytest.raises(SystemExit):
        train.parse_args(["--ppr-select", "lists"])
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--ppr-eps", "1e-4", "--ppr-select", "rows"])


# ---- the numpy reference itself ----------------------------------------------------------------


def _path3():
    a = sp.csr_matrix(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=np.float32))
    at = sp.csr_matrix(O.calc_a_hat(a, "sym").astype(np.float32))
    return at


def test_reference_pads_a_short_row_with_the_smallest_free_indices():
    at = _path3()
    # one round from node 2: p = alpha at node 2 only, so k = 2 keeps node 2 and pads with node 0
    idx, val, rounds, left, V = push_topk_ref.push_topk(at.indptr, at.indices, at.data, [2, 7, 0],
                                                        ALPHA, 1e-4, 2, max_rounds=1)
    a = np.float64(np.float32(ALPHA))
    want = np.float32(np.float64(int(2.0 ** 44 * a)) * 2.0 ** -44)
    assert idx.dtype == np.int32 and val.dtype == np.float32
    assert idx.tolist() == [[0, 2], [0, 1], [0, 1]]
    assert val[0].tolist() == [0.0, want] and val[2].tolist() == [want, 0.0]
    assert not val[1].any() and not np.signbit(val).any()
    assert list(rounds) == [1, 0, 1] and left[1] == -1 and left[0] > 0
    short, tied = push_topk_ref.short_and_tied(V, 2)
    assert short.all() and not tied.any()


def test_reference_orders_on_the_scaled_value_and_breaks_ties_by_index():
    V = np.array([[1.0, 2.0], [3.0, 2.0], [3.0, 2.0], [0.5, 2.0]], dtype=np.float32)
    idx, val = push_topk_ref.select(V, 2)
    assert idx.tolist() == [[1, 2], [0, 1]]  # column 1: all tied, the lowest indices win
    assert val.tolist() == [[3.0, 3.0], [2.0, 2.0]]
    short, tied = push_topk_ref.short_and_tied(V, 2)
    assert not short.any() and tied.tolist() == [False, True]
    # the row scale changes the order: the candidate is the product, rounded in fp32
    rs = np.array([8.0, 1.0, 0.25, 1.0], dtype=np.float32)
    idx, val = push_topk_ref.select(push_topk_ref.candidates(V, rs, None), 2)
    assert idx[0].tolist() == [0, 1] and val[0].tolist() == [8.0, 3.0]


def test_reference_equals_the_replay_block_selected_by_hand():
    at = _path3()
    X, rounds, left, _ = push_ref.push_columns(at.indptr, at.indices, at.data, [1, 0], ALPHA, 1e-4)
    idx, val, r2, l2, V = push_topk_ref.push_topk(at.indptr, at.indices, at.data, [1, 0], ALPHA,
                                                  1e-4, 3)
    assert np.array_equal(V.view(np.uint32), X.view(np.uint32))
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2]]  # k = n: every node, in order
    assert np.array_equal(val.view(np.uint32), np.ascontiguousarray(X.T).view(np.uint32))
    assert np.array_equal(rounds, r2) and np.array_equal(left, l2)
