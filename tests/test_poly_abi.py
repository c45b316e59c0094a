"""CPU: the ABI of the polynomial propagation (appnp_poly, include/ppnp_amd.h) and its reference.

No compute call is made (there is no GPU here): the exports, the argument validation that returns
before touching the device, the workspace size, the coefficient helpers against their closed
forms, and the fp64 reference of the GPU tests (tests/poly_ref.py) against the oracle's APPNP
series, which it must equal with the PPR coefficients.
"""

import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ppnp_oracle as O

import poly_ref


def _lib():
    from ppnp_amd import _lib

    return _lib, _lib.load()


def test_poly_symbols_exported():
    L, lib = _lib()
    for name in ("appnp_poly_workspace_bytes", "appnp_poly", "appnp_poly_bwd"):
        assert name in L.EXPORTED
        assert hasattr(lib, name)
    assert lib.appnp_abi_version() == L.ABI_VERSION == 2  # a backward-compatible addition
    import ppnp_amd
    from ppnp_amd import ops

    for name in ("poly", "poly_forward", "poly_backward", "ppr_coefficients", "heat_coefficients",
                 "GPRGNN"):
        assert hasattr(ppnp_amd, name), name
    assert ops.POLY_MAX_K == 1024


class _GraphHead(C.Structure):
    """The leading fields of struct appnp_graph (ppnp_amd/csrc/appnp_internal.h), followed by
    zero bytes for the rest (every pointer NULL, no transpose): a host-only stand-in that the
    validation reads and no device call ever sees."""
    _fields_ = [("n", C.c_int64), ("row_lo", C.c_int64), ("row_hi", C.c_int64),
                ("nnz_hat", C.c_int64), ("nnz_local", C.c_int64), ("nnz_remote", C.c_int64),
                ("mode", C.c_int), ("symmetric", C.c_int), ("rest", C.c_char * 2048)]


def _graph(n=100, row_lo=0, row_hi=None, mode=0, symmetric=1):
    return _GraphHead(n=n, row_lo=row_lo, row_hi=n if row_hi is None else row_hi, mode=mode,
                      symmetric=symmetric)


def _gp(g):
    return None if g is None else C.cast(C.pointer(g), C.c_void_p)


P, Q, R = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)  # never dereferenced
BIG = 1 << 50


def test_poly_forward_validation_without_device():
    """Every case returns its code before any device call, in the order of appnp_solve."""
    L, lib = _lib()
    full = _graph()

    def call(g=full, H=P, ld_h=8, Z=Q, ld_z=8, f=7, dtype=L.F32, K=4, coef=R, ws=P,
             ws_bytes=BIG):
        return lib.appnp_poly(_gp(g), H, ld_h, Z, ld_z, f, dtype, K, coef, ws, ws_bytes, None)

    E, OK, NS = L.APPNP_EINVAL, L.APPNP_OK, L.APPNP_ENOTSUP
    assert call(g=None) == E
    assert call(f=-1) == E
    assert call(f=2**31) == E
    assert call(K=-1) == E
    assert call(K=1025) == E
    assert call(dtype=7) == E
    assert call(g=_graph(row_lo=10)) == E           # needs the whole graph
    assert call(g=_graph(row_hi=50)) == E
    assert call(g=_graph(row_hi=50), dtype=L.BF16) == E  # the partition is checked first
    assert call(dtype=L.BF16) == NS
    assert call(dtype=L.BF16, H=None) == NS              # ... and bf16 before the pointers
    # the forward runs on any full graph: rw, directed, no transpose needed.  Up to here every
    # check passed: what fails below is the pointers
    for g in (_graph(mode=1), _graph(symmetric=0), _graph(mode=1, symmetric=0)):
        assert call(g=g, H=None) == E
        assert call(g=g, f=0, H=None, Z=None, coef=None, ws=None, ws_bytes=0) == OK
    # empty shapes: nothing to do, whatever the pointers are -- but only after the checks above
    assert call(g=_graph(n=0), H=None, Z=None, coef=None, ws=None, ws_bytes=0) == OK
    assert call(f=0, H=None, Z=None, coef=None, ws=None, ws_bytes=0) == OK
    assert call(f=0, K=1025) == E
    assert call(g=_graph(n=0), dtype=L.BF16) == NS
    assert call(H=None) == E
    assert call(Z=None) == E
    assert call(coef=None) == E
    assert call(ld_h=6) == E
    assert call(ld_z=6) == E
    assert call(Z=P) == E                                 # H == Z
    # the workspace: none for K <= 1, else appnp_poly_workspace_bytes
    need = lib.appnp_poly_workspace_bytes(_gp(full), 7, 4, 0)
    assert need > 0
    assert call(ws=None) == E
    assert call(ws_bytes=0) == E
    assert call(ws_bytes=need - 257) == E


def test_poly_backward_validation_without_device():
    L, lib = _lib()
    full = _graph()
    S = C.c_void_p(0x4000)

    def call(g=full, dZ=P, ld_dz=8, H=S, ld_h=8, dH=Q, ld_dh=8, dcoef=R, f=7, dtype=L.F32, K=4,
             coef=R, ws=P, ws_bytes=BIG):
        return lib.appnp_poly_bwd(_gp(g), dZ, ld_dz, H, ld_h, dH, ld_dh, dcoef, f, dtype, K, coef,
                                  ws, ws_bytes, None)

    E, OK, NS = L.APPNP_EINVAL, L.APPNP_OK, L.APPNP_ENOTSUP
    assert call(g=None) == E
    assert call(f=-1) == E
    assert call(K=-1) == E
    assert call(K=1025) == E
    assert call(dtype=7) == E
    assert call(g=_graph(row_lo=10)) == E
    assert call(g=_graph(row_lo=10), dtype=L.BF16) == E
    assert call(dtype=L.BF16) == NS
    # A_hat^T: A_hat itself for sym on a symmetric graph, else the transpose, which the stand-in
    # does not have
    assert call(g=_graph(mode=1)) == NS
    assert call(g=_graph(symmetric=0)) == NS
    assert call(g=_graph(mode=1, symmetric=0)) == NS
    assert call(g=_graph(mode=1), f=0) == NS            # before the empty shape
    assert call(g=_graph(row_hi=50, mode=1)) == E       # after the partition
    assert call(f=0, dZ=None, H=None, dH=None, dcoef=None, coef=None, ws=None, ws_bytes=0) == OK
    assert call(g=_graph(n=0), dZ=None, H=None, dH=None, coef=None, ws=None, ws_bytes=0) == OK
    assert call(dZ=None) == E
    assert call(dH=None) == E
    assert call(coef=None) == E
    assert call(ld_dz=6) == E
    assert call(ld_dh=6) == E
    assert call(dH=P) == E                                # dZ == dH
    # H is needed for the dots only
    assert call(H=None) == E
    assert call(ld_h=6) == E
    assert call(H=Q) == E                                 # H == dH
    assert call(H=None, dcoef=None, ws_bytes=0) == E      # past H: only the workspace is missing
    assert call(H=None, ld_h=0, dcoef=None, ws=None) == E
    for with_dcoef in (0, 1):
        need = lib.appnp_poly_workspace_bytes(_gp(full), 7, 4, with_dcoef)
        assert call(dcoef=R if with_dcoef else None, ws_bytes=need - 257) == E
    # K = 0 with the dots still needs the partials
    assert lib.appnp_poly_workspace_bytes(_gp(full), 7, 0, 1) > 0
    assert call(K=0, ws=None, ws_bytes=0) == E


def test_poly_workspace_bytes_monotone_and_empty():
    _, lib = _lib()
    ws = lib.appnp_poly_workspace_bytes
    g = _gp(_graph(n=2995))
    assert ws(None, 8, 4, 1) == 0
    assert ws(_gp(_graph(n=0)), 8, 4, 1) == 0
    assert ws(g, 0, 4, 1) == 0 and ws(g, -1, 4, 1) == 0
    assert ws(g, 8, -1, 1) == 0 and ws(g, 8, 1025, 1) == 0
    # K <= 1 keeps no power in a buffer; without the dots that is no workspace at all
    assert ws(g, 8, 0, 0) == 0 and ws(g, 8, 1, 0) == 0
    fs = list(range(1, 301)) + [512, 1000, 4096]
    ks = [0, 1, 2, 3, 4, 10, 100, 1024]
    for wd in (0, 1):
        for k in ks:
            sizes = [ws(g, f, k, wd) for f in fs]
            assert sizes == sorted(sizes), (wd, k)
        for f in (1, 3, 64, 65, 100, 260):
            sizes = [ws(g, f, k, wd) for k in ks]
            assert sizes == sorted(sizes), (wd, f)
            assert sizes[3] == sizes[-1]  # two buffers from K = 3 on
    for f in (1, 64, 65, 130, 260):
        for k in ks:
            # the partial dots: one fp32 per (64-column slab, row) at the least
            assert ws(g, f, k, 1) - ws(g, f, k, 0) >= 4 * 2995 * ((f + 63) // 64)
    assert ws(g, 16, 10, 0) >= 2 * 2995 * 16 * 4


@pytest.mark.parametrize("K,alpha", [(0, 0.1), (1, 0.1), (10, 0.1), (10, 0.2), (64, 0.05),
                                     (5, 1.0), (5, 0.0)])
def test_ppr_coefficients_closed_form(K, alpha):
    import ppnp_amd

    g = ppnp_amd.ppr_coefficients(K, alpha)
    assert g.dtype.is_floating_point and g.element_size() == 4 and tuple(g.shape) == (K + 1,)
    want = np.array([alpha * (1 - alpha) ** k for k in range(K)] + [(1 - alpha) ** K])
    assert np.array_equal(g.numpy(), want.astype(np.float32))
    assert float(g[-1]) == np.float32((1 - alpha) ** K)
    assert abs(float(g.double().sum()) - 1.0) <= (K + 1) * 2.0 ** -24
    assert np.allclose(poly_ref.ppr_coefficients(K, alpha), want, rtol=1e-15, atol=0)


@pytest.mark.parametrize("K,t", [(0, 1.0), (10, 1.0), (10, 3.0), (20, 0.5), (4, 0.0)])
def test_heat_coefficients_closed_form(K, t):
    import ppnp_amd

    g = ppnp_amd.heat_coefficients(K, t)
    assert tuple(g.shape) == (K + 1,) and g.element_size() == 4
    want = np.array([math.exp(-t) * t ** k / math.factorial(k) for k in range(K + 1)])
    assert np.allclose(g.double().numpy(), want, rtol=2e-7, atol=1e-30)
    assert np.allclose(poly_ref.heat_coefficients(K, t), want, rtol=1e-15, atol=0)
    assert float(g.double().sum()) <= 1.0 + 1e-6


def adj_of(g):
    n = int(g["n"])
    return sp.csr_matrix((g["adj_data"], g["adj_indices"], g["adj_indptr"]), shape=(n, n))


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_reference_with_ppr_coefficients_is_the_appnp_series(cora, mode):
    a = poly_ref.a_hat(adj_of(cora), mode)
    H = cora["H"].astype(np.float64)
    K, alpha = 10, 0.1
    coef = poly_ref.ppr_coefficients(K, alpha)
    ref = O.appnp_propagate(a, H, K, alpha)
    err = np.abs(poly_ref.forward(a, H, coef) - ref).max()
    print(f"{mode}: |poly_ref - appnp_propagate| = {err:.2e}")
    assert err <= 1e-14 * np.abs(ref).max()
    dZ = np.random.default_rng(3).standard_normal(H.shape)
    dH, dcoef, S = poly_ref.backward(a, dZ, H, coef)
    dref = O.appnp_backward(a, dZ, K, alpha)
    assert np.abs(dH - dref).max() <= 1e-14 * np.abs(dref).max()
    # d gamma_k = <dZ, A_hat^k H>: the definition, term by term
    t = H
    for k in range(K + 1):
        assert abs(dcoef[k] - (dZ * t).sum()) <= 1e-12 * S[k]
        assert S[k] >= abs(dcoef[k])
        t = a @ t


def test_poly_ops_on_meta_tensors():
    import torch

    import ppnp_amd  # noqa: F401  (registers the ops)

    H = torch.empty(11, 7, device="meta")
    coef = torch.empty(5, device="meta")
    Z = torch.ops.ppnp_amd.poly(H, coef, 1)
    assert Z.shape == H.shape and Z.dtype == H.dtype and Z.device.type == "meta"
    dH, dcoef = torch.ops.ppnp_amd.poly_bwd(Z, H, coef, 1, True)
    assert dH.shape == H.shape and dcoef.shape == coef.shape
    dH, dcoef = torch.ops.ppnp_amd.poly_bwd(Z, H, coef, 1, False)
    assert dH.shape == H.shape and dcoef.numel() == 0


def test_gprgnn_surface():
    import torch

    from ppnp_amd import GPRGNN, ppr_coefficients, heat_coefficients

    adj = sp.csr_matrix(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=np.float32))
    m = GPRGNN(4, 2, adj, K=6, alpha=0.2)
    assert isinstance(m.coef, torch.nn.Parameter) and m.coef.requires_grad
    assert torch.equal(m.coef.detach(), ppr_coefficients(6, 0.2))
    assert all(p is not m.coef for p in m._reg_params)  # gamma is not in the L2 term
    assert "coef" in dict(m.named_parameters())
    fixed = GPRGNN(4, 2, adj, K=6, init="heat", heat_t=2.0, learn_coef=False)
    assert "coef" not in dict(fixed.named_parameters()) and "coef" in dict(fixed.named_buffers())
    assert torch.equal(fixed.coef, heat_coefficients(6, 2.0))
    given = GPRGNN(4, 2, adj, K=2, init=torch.tensor([1.0, -0.5, 0.0]))
    assert given.coef.detach().tolist() == [1.0, -0.5, 0.0]
    with pytest.raises(ValueError):
        GPRGNN(4, 2, adj, K=3, init=torch.ones(3))
    with pytest.raises(ValueError):
        GPRGNN(4, 2, adj, init="cheb")
    with pytest.raises(Exception):
        m(torch.zeros(3, 4))  # model.py:66-67, as APPNP


def test_trainer_takes_gprgnn():
    from ppnp_amd import train

    a = train.parse_args(["--model", "gprgnn", "--coef-init", "heat", "--heat-t", "2",
                          "--fixed-coef"])
    assert a.model == "gprgnn" and a.coef_init == "heat" and a.heat_t == 2.0 and a.fixed_coef
    d = train.parse_args([])
    assert d.model == "appnp" and d.coef_init == "ppr" and not d.fixed_coef  # defaults unchanged
    with pytest.raises(SystemExit):
        train.parse_args(["--model", "gprgnn", "--edge-drop", "0.1"])
    with pytest.raises(SystemExit):
        train.parse_args(["--model", "gprgnn", "--batch-size", "32", "--ppr-topk", "32"])
