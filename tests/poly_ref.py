"""fp64 reference of the polynomial propagation Z = sum_k gamma_k A_hat^k H (appnp_poly).

numpy / scipy on the oracle's ``calc_a_hat``; what tests/test_poly_abi.py checks against the
oracle's APPNP series and tests/test_gpu_poly.py compares the kernels with.
"""

import numpy as np

from oracle import ppnp_oracle as O


def a_hat(adj, mode="sym"):
    """The oracle's A_hat as an fp64 CSR."""
    return O.calc_a_hat(adj, mode).astype(np.float64).tocsr()


def forward(a, H, coef):
    """Z = sum_k coef[k] a^k H."""
    t = np.asarray(H, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    z = coef[0] * t
    for c in coef[1:]:
        t = a @ t
        z = z + c * t
    return z


def backward(a, dZ, H, coef):
    """(dH, dcoef, S) of ``forward`` for the cotangent dZ: with G_0 = dZ, G_k = a^T G_{k-1},
    dH = sum_k coef[k] G_k, dcoef[k] = <G_k, H> and S[k] = sum |G_k o H|, the sum of the absolute
    terms of that dot: the scale its rounding error is measured in."""
    g = np.asarray(dZ, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    at = a.T.tocsr()
    dH = coef[0] * g
    dcoef, S = [float((g * H).sum())], [float(np.abs(g * H).sum())]
    for c in coef[1:]:
        g = at @ g
        dH = dH + c * g
        dcoef.append(float((g * H).sum()))
        S.append(float(np.abs(g * H).sum()))
    return dH, np.array(dcoef), np.array(S)


def ppr_coefficients(K, alpha):
    """alpha (1-alpha)^k for k < K, (1-alpha)^K last: the K-step APPNP series."""
    g = alpha * (1.0 - alpha) ** np.arange(K + 1, dtype=np.float64)
    g[K] = (1.0 - alpha) ** K
    return g


def heat_coefficients(K, t):
    """e^-t t^k / k!."""
    from math import exp, factorial

    return np.array([exp(-t) * t ** k / factorial(k) for k in range(K + 1)])
