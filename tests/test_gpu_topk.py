"""GPU: appnp_topk_columns against a numpy reference, bit for bit.

The reference works on the same fp32 array: the candidate v = (X * row_scale) * col_scale in
fp32, a stable argsort of (-v, row) under the header's total order (-0 == +0, NaN below every
number, ties to the smaller row), the first k, sorted by row.  The rule is total, so no case is
excluded and every comparison is exact (values compared as their bit patterns).

Every call runs with padded leading dimensions: ld_x = b + 5 with +inf in the padding (a kernel
that read it would select it), ld_out = k + 3 with sentinel-filled buffers; both paddings must
come back untouched.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import ppnp_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDX_SENTINEL, VAL_SENTINEL = -7, 777.0
NS = [1, 63, 64, 65, 1000, 70_001]
BS = [1, 7, 31, 32, 33, 128, 130]
KS = [1, 2, 31, 64, 128, "n"]


def reference(V, k):
    """(idx [b, k] int32, val [b, k] fp32) of the fp32 candidates V [n, b]."""
    n, b = V.shape
    w = V.astype(np.float64)
    w[np.isneginf(V)] = -1.0e300     # below every finite fp32, above NaN
    w[np.isnan(V)] = -np.inf
    idx = np.empty((b, k), dtype=np.int32)
    for c in range(b):
        order = np.argsort(-w[:, c], kind="stable")[:k]  # -0.0 == 0.0: ties keep row order
        idx[c] = np.sort(order)
    val = np.ascontiguousarray(V.T)[np.arange(b)[:, None], idx]
    return idx, val


def candidates(X, rs, cs):
    V = X
    if rs is not None:
        V = V * rs[:, None]
    if cs is not None:
        V = V * cs[None, :]
    assert V.dtype == np.float32
    return V


class Call:
    """One shape's device buffers, padded as the module docstring says."""

    def __init__(self, X, k, rs=None, cs=None):
        from ppnp_amd import _lib

        self.L, self.lib = _lib, _lib.load()
        self.n, self.b, self.k = X.shape[0], X.shape[1], int(k)
        self.ld_x, self.ld_out = self.b + 5, self.k + 3
        self.host = np.full((self.n, self.ld_x), np.inf, dtype=np.float32)
        self.host[:, :self.b] = X
        self.X = torch.from_numpy(self.host).to(DEV)
        self.rs = None if rs is None else torch.from_numpy(rs).to(DEV)
        self.cs = None if cs is None else torch.from_numpy(cs).to(DEV)
        self.idx = torch.full((self.b, self.ld_out), IDX_SENTINEL, dtype=torch.int32, device=DEV)
        self.val = torch.full((self.b, self.ld_out), VAL_SENTINEL, dtype=torch.float32,
                              device=DEV)
        self.ws_bytes = int(self.lib.appnp_topk_workspace_bytes(self.n, self.b, self.k))
        self.ws = torch.empty(max(self.ws_bytes, 1), dtype=torch.uint8, device=DEV)

    def launch(self):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        rc = self.lib.appnp_topk_columns(
            p(self.X), self.ld_x, self.n, self.b, self.k, p(self.rs), p(self.cs), p(self.idx),
            p(self.val), self.ld_out, p(self.ws), self.ws_bytes,
            C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == self.L.APPNP_OK, rc

    def result(self):
        """(idx, val bits) after checking that neither padding was written."""
        idx, val = self.idx.cpu().numpy(), self.val.cpu().numpy()
        assert (idx[:, self.k:] == IDX_SENTINEL).all(), "out_idx padding written"
        assert (val[:, self.k:] == VAL_SENTINEL).all(), "out_val padding written"
        assert np.array_equal(self.X.cpu().numpy().view(np.uint32), self.host.view(np.uint32))
        return idx[:, :self.k], np.ascontiguousarray(val[:, :self.k]).view(np.uint32)


def check(X, k, rs=None, cs=None, tag=""):
    call = Call(X, k, rs, cs)
    call.launch()
    torch.cuda.synchronize()
    idx, bits = call.result()
    ridx, rval = reference(candidates(X, rs, cs), k)
    assert np.array_equal(idx, ridx), f"{tag} n={X.shape[0]} b={X.shape[1]} k={k}: indices"
    assert np.array_equal(bits, rval.view(np.uint32)), \
        f"{tag} n={X.shape[0]} b={X.shape[1]} k={k}: values"
    return call


# ---------------------------------------------------------------------------------------
# (a) N(0, 1) over the shape grid
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", NS[:-1])
def test_shape_grid_normal(n):
    """Every b and every valid k at the small n (sub-block edges 63 / 64 / 65, more than one row
    block at 1000 with a partial last sub-block)."""
    rng = np.random.default_rng(n)
    for b in BS:
        X = rng.standard_normal((n, b)).astype(np.float32)
        for k in sorted({n if k == "n" else k for k in KS if k == "n" or k <= n}):
            check(X, k, tag="normal")


# n = 70 001: 547 sub-blocks, the last of 113 rows; thinned, b = 33 / 130 kept, every k once
BIG = [(1, 64), (7, 31), (33, 1), (33, 2), (33, "n"), (130, 128), (32, 128)]


@pytest.mark.parametrize("b,k", BIG)
def test_large_n_normal(b, k):
    n = NS[-1]
    X = np.random.default_rng(1000 * b).standard_normal((n, b)).astype(np.float32)
    check(X, n if k == "n" else k, tag="normal")


def test_scales_are_applied_in_order():
    rng = np.random.default_rng(5)
    n, b = 1000, 33
    X = rng.standard_normal((n, b)).astype(np.float32)
    rs = rng.uniform(0.5, 40.0, n).astype(np.float32)
    cs = rng.uniform(0.01, 2.0, b).astype(np.float32)
    check(X, 31, rs, cs, tag="scales")
    check(X, 31, rs, None, tag="row scale")
    check(X, 31, None, cs, tag="col scale")


# ---------------------------------------------------------------------------------------
# (b) - (e) ties, radix digits, special values
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,b,k", [(65, 7, 31), (1000, 33, 64), (70_001, 130, 128)])
def test_four_distinct_values(n, b, k):
    X = np.random.default_rng(n).choice(
        np.array([-1.5, 0.0, 0.25, 3.0], dtype=np.float32), size=(n, b))
    check(X, k, tag="4 values")


def test_whole_column_equal_cuts_the_tie_across_row_blocks():
    n, b, k = 70_001, 33, 40_000
    X = np.full((n, b), 0.375, dtype=np.float32)
    call = check(X, k, tag="equal")
    idx, _ = call.result()
    assert np.array_equal(idx, np.broadcast_to(np.arange(k, dtype=np.int32), (b, k)))


@pytest.mark.parametrize("digit", [0, 1, 2, 3])
def test_one_case_per_radix_digit(digit):
    """Candidates that differ only in byte ``digit`` of their bit pattern (base + i ulps scaled
    to that byte), so that pass of the radix select alone decides; 1000 rows over 256 values
    leave ties in every column.  Byte 3 flips the sign and the high exponent bits (bit 23 of the
    base is clear, so no pattern is an inf or a NaN)."""
    n, b, k = 1000, 33, 100
    rng = np.random.default_rng(digit)
    base = np.uint32(0x3E345678) & ~np.uint32(0xFF << (8 * digit))
    i = np.stack([rng.permutation(n) for _ in range(b)], axis=1).astype(np.uint32)
    bits = base | ((i % 256) << np.uint32(8 * digit))
    X = np.ascontiguousarray(bits.astype(np.uint32)).view(np.float32)
    assert np.isfinite(X).all()
    check(X, k, tag=f"digit {digit}")


@pytest.mark.parametrize("k", [31, 995, 998, 1000])
def test_special_values(k):
    """+-0, negatives, subnormals, +-inf and a few NaNs (5 per column: k = 998 cuts inside the
    NaNs, k = 995 right above them)."""
    n, b = 1000, 7
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, b)).astype(np.float32)
    tiny = np.float32(1e-45)
    specials = np.array([0.0, -0.0, 0.0, -0.0, tiny, -tiny, 3 * tiny, np.float32(1e-39),
                         -np.float32(1e-39), np.inf, np.inf, -np.inf, -np.inf, np.nan, np.nan,
                         np.nan, -np.nan, np.nan], dtype=np.float32)
    assert np.isnan(specials).sum() == 5
    for c in range(b):
        X[rng.choice(n, len(specials), replace=False), c] = specials
    check(X, k, tag="specials")


# ---------------------------------------------------------------------------------------
# (f) PPR columns of Cora-ML from the fp64 oracle
# ---------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def cora_ppr(cora):
    n = int(cora["n"])
    adj = sp.csr_matrix((cora["adj_data"], cora["adj_indices"], cora["adj_indptr"]), shape=(n, n))
    idx = np.sort(np.random.default_rng(3).choice(n, 130, replace=False))
    deg = np.asarray(adj.sum(axis=1)).ravel() + 1.0
    out = {"idx": idx, "deg": deg}
    for mode in ("sym", "rw"):
        out[mode] = np.ascontiguousarray(O.compute_ppr(adj, 0.1, mode)[:, idx].astype(np.float32))
    return out


@pytest.mark.parametrize("k", [8, 32, 128])
def test_cora_ppr_columns_sym(cora_ppr, k):
    check(cora_ppr["sym"], k, tag="cora sym")


@pytest.mark.parametrize("k", [8, 128])
def test_cora_ppr_columns_rw_with_scales(cora_ppr, k):
    """rw: Pi[i, :] = D * Pi[:, i] / d_i as the kernel's row and column scales."""
    deg, idx = cora_ppr["deg"], cora_ppr["idx"]
    check(cora_ppr["rw"], k, deg.astype(np.float32), (1.0 / deg[idx]).astype(np.float32),
          tag="cora rw")


# ---------------------------------------------------------------------------------------
# determinism, graph capture, the torch-level wrapper
# ---------------------------------------------------------------------------------------


def test_two_runs_are_bit_identical():
    X = np.random.default_rng(2).choice(
        np.array([0.5, 0.25, 1.0], dtype=np.float32), size=(70_001, 33))
    a, b = Call(X, 128), Call(X, 128)
    a.launch()
    b.launch()
    a.launch()  # and a second run over a used workspace
    torch.cuda.synchronize()
    (ia, va), (ib, vb) = a.result(), b.result()
    assert np.array_equal(ia, ib) and np.array_equal(va, vb)


def test_graph_capture_replays_after_refill():
    """The chain is a linear sequence of launches on one stream: captured once, it replays to the
    result of the data then in X."""
    rng = np.random.default_rng(4)
    n, b, k = 1000, 33, 31
    X0 = rng.standard_normal((n, b)).astype(np.float32)
    X1 = rng.standard_normal((n, b)).astype(np.float32)
    call = Call(X0, k)
    call.launch()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call.launch()
    for X in (X0, X1):
        call.host[:, :b] = X
        call.X.copy_(torch.from_numpy(call.host))
        call.idx.fill_(IDX_SENTINEL)
        call.val.fill_(VAL_SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        idx, bits = call.result()
        ridx, rval = reference(X, k)
        assert np.array_equal(idx, ridx) and np.array_equal(bits, rval.view(np.uint32))


def test_ops_topk_columns_wrapper_passes_a_padded_ld_through():
    from ppnp_amd.ops import topk_columns

    rng = np.random.default_rng(6)
    n, b, k = 1000, 33, 64
    host = rng.standard_normal((n, b + 7)).astype(np.float32)
    Xp = torch.from_numpy(host).to(DEV)
    rs = rng.uniform(0.5, 2.0, n).astype(np.float32)
    idx, val = topk_columns(Xp[:, :b], k, row_scale=torch.from_numpy(rs).to(DEV))
    assert idx.shape == (b, k) and idx.dtype == torch.int32 and val.dtype == torch.float32
    ridx, rval = reference(candidates(np.ascontiguousarray(host[:, :b]), rs, None), k)
    assert np.array_equal(idx.cpu().numpy(), ridx)
    assert np.array_equal(val.cpu().numpy().view(np.uint32), rval.view(np.uint32))
    with pytest.raises(ValueError):
        topk_columns(Xp[:, :b], n + 1)
