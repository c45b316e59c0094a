"""CPU: the host-only part of the exact PPNP solver (include/ppnp_amd.h appnp_solve*).

The iteration count and the Chebyshev weights are computed on the host, so the recurrence the
GPU kernels run can be replayed here in numpy, in fp64, against the reference fixtures
(pprH_a0.1 = compute_ppr(adj, 0.1) @ H, helpers.py:68-71).  No compute call reaches a device.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp


def _lib():
    from ppnp_amd import _lib

    return _lib


def iterations(alpha, tol):
    lib = _lib().load()
    m = C.c_int(-1)
    return lib.appnp_solve_iterations(alpha, tol, C.byref(m)), m.value


@pytest.mark.parametrize("alpha,tol,want", [
    (0.1, 1e-3, 17), (0.1, 1e-5, 27), (0.1, 1e-6, 32), (0.1, 1e-7, 36),
    (0.2, 1e-3, 11), (0.2, 1e-5, 18), (0.2, 1e-7, 25),
    (1.0, 1e-3, 1), (1.0, 1e-7, 1), (1.0, 0.5, 1)])
def test_iteration_counts(alpha, tol, want):
    assert iterations(alpha, tol) == (0, want)
    import ppnp_amd

    assert ppnp_amd.solve_iterations(alpha, tol) == want


def test_iteration_count_is_the_smallest_that_meets_the_bound():
    for alpha in (0.05, 0.1, 0.2, 0.5):
        rho = 1.0 - float(np.float32(alpha))
        sigma = rho / (1.0 + np.sqrt(1.0 - rho * rho))
        for tol in (1e-2, 1e-4, 1e-6):
            rc, m = iterations(alpha, tol)
            assert rc == 0
            bound = lambda k: 2 * sigma ** k / (1 + sigma ** (2 * k))  # noqa: E731
            assert bound(m) <= float(np.float32(tol))
            assert m == 1 or bound(m - 1) > float(np.float32(tol))


@pytest.mark.parametrize("alpha,tol", [(0.0, 1e-6), (-0.1, 1e-6), (1.5, 1e-6), (float("nan"), 1e-6),
                                       (0.1, 0.0), (0.1, 1.0), (0.1, -1e-3), (0.1, float("nan"))])
def test_iterations_reject_bad_alpha_or_tol(alpha, tol):
    L = _lib()
    assert iterations(alpha, tol)[0] == L.APPNP_EINVAL
    assert L.load().appnp_solve_iterations(0.1, 1e-6, None) == L.APPNP_EINVAL


def test_weights_follow_the_recurrence():
    L = _lib()
    lib = L.load()
    w = (C.c_double * 40)()
    assert lib.appnp_solve_weights(0.1, 40, w) == 0
    rho2 = (1.0 - float(np.float32(0.1))) ** 2
    assert w[0] == 1.0
    assert w[1] == pytest.approx(1.0 / (1.0 - rho2 / 2), rel=1e-15)
    for k in range(2, 40):
        assert w[k] == pytest.approx(1.0 / (1.0 - rho2 * w[k - 1] / 4), rel=1e-15)
    # the weights fall towards 1 + sigma^2
    sigma = np.sqrt(rho2) / (1.0 + np.sqrt(1.0 - rho2))
    assert w[39] == pytest.approx(1 + sigma ** 2, rel=1e-9)
    assert lib.appnp_solve_weights(0.1, 0, w) == L.APPNP_EINVAL
    assert lib.appnp_solve_weights(0.0, 4, w) == L.APPNP_EINVAL
    assert lib.appnp_solve_weights(0.1, 4, None) == L.APPNP_EINVAL


def test_solve_rejects_a_null_graph_before_any_device_call():
    L = _lib()
    lib = L.load()
    buf = C.c_void_p(0x1000)
    for fn in (lib.appnp_solve, lib.appnp_solve_bwd):
        assert fn(None, buf, 8, C.c_void_p(0x2000), 8, 7, L.F32, 32, 0.1, None, 0,
                  None) == L.APPNP_EINVAL
    out = C.c_void_p()
    assert lib.appnp_plan_create_solve(None, buf, 8, C.c_void_p(0x2000), 8, 7, L.F32, 32, 0.1,
                                       None, 0, C.byref(out)) == L.APPNP_EINVAL
    assert out.value is None


def a_hat_of(g, mode):
    n = int(g["n"])
    return sp.csr_matrix((g[f"ahat_{mode}_data"], g[f"ahat_{mode}_indices"],
                          g[f"ahat_{mode}_indptr"]), shape=(n, n))


def chebyshev_replay(a_hat, H, alpha, omega):
    """The recurrence of appnp_solve in fp64 with the library's weights."""
    H = np.asarray(H, dtype=np.float64)
    prev, z = None, H
    for w in omega:
        t = (1.0 - alpha) * (a_hat @ z) + alpha * H
        prev, z = z, (t if prev is None else w * t + (1.0 - w) * prev)
    return z


@pytest.mark.parametrize("mode,key", [("sym", "pprH_a0.1"), ("rw", "pprH_rw_a0.1")])
def test_replay_reaches_the_reference_where_the_plain_series_does_not(cora, mode, key):
    import ppnp_amd
    from oracle import ppnp_oracle as O

    alpha, tol = 0.1, 1e-6
    m = ppnp_amd.solve_iterations(alpha, tol)
    assert m == 32
    from ppnp_amd.ops import solve_weights

    omega = solve_weights(alpha, m)
    a_hat = a_hat_of(cora, mode)
    ref = cora[key]
    bar = 1e-5 * np.abs(ref).max()
    err = np.abs(chebyshev_replay(a_hat, cora["H"], alpha, omega) - ref).max()
    plain = np.abs(O.appnp_propagate(a_hat, cora["H"].astype(np.float64), m, alpha) - ref).max()
    print(f"{mode}: chebyshev m={m} err {err:.3e}, plain series K={m} err {plain:.3e}, "
          f"bar {bar:.3e}")
    assert err <= bar
    assert plain > bar  # the acceleration, not the count, is what passes


def test_solve_op_on_meta_tensors():
    import torch

    import ppnp_amd  # noqa: F401  (registers the ops)

    H = torch.empty(11, 7, device="meta")
    Z = torch.ops.ppnp_amd.solve(H, 1, 32, 0.1)
    assert Z.shape == H.shape and Z.dtype == H.dtype and Z.device.type == "meta"
    dH = torch.ops.ppnp_amd.solve_bwd(Z, 1, 32, 0.1)
    assert dH.shape == H.shape and dH.dtype == H.dtype


def test_model_exact_flag():
    import torch

    from ppnp_amd import APPNP

    adj = sp.csr_matrix(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=np.float32))
    with pytest.raises(ValueError):
        APPNP(4, 2, adj, exact=True, edge_drop=0.1)
    plain, exact = APPNP(4, 2, adj), APPNP(4, 2, adj, exact=True, tol=1e-5)
    assert plain.exact is False and exact.exact is True and exact.tol == 1e-5
    X = torch.zeros(3, 4)
    with torch.no_grad():
        plain.eval(), exact.eval()
        kp, ke = plain._memo_key(X), exact._memo_key(X)
    assert kp[-2:] == (False, 1e-6) and ke[-2:] == (True, 1e-5)
