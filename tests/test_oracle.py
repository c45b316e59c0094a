"""CPU: pin the oracle (oracle/ppnp_oracle.py) to the reference's golden vectors.

The fixtures in tests/golden/ were produced by tests/golden/make_golden.py from the
reference's own helpers.calc_A_hat / compute_ppr / model.PPNP / SparseGraph.standardize.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import ppnp_oracle as O


def adj_of(g, prefix="adj"):
    n = int(g["n"]) if prefix == "adj" else int(g["adj_raw_n"])
    return sp.csr_matrix((g[f"{prefix}_data"], g[f"{prefix}_indices"], g[f"{prefix}_indptr"]),
                         shape=(n, n))


@pytest.mark.parametrize("ds", ["cora", "citeseer"])
def test_standardize_matches_reference(ds, request):
    g = request.getfixturevalue(ds)
    a, keep = O.standardize(adj_of(g, "adj_raw"), select_lcc=True)
    ref = adj_of(g)
    assert a.shape == ref.shape
    assert np.array_equal(a.indptr, ref.indptr)
    assert np.array_equal(a.indices, ref.indices)
    assert np.all(a.data == 1)


@pytest.mark.parametrize("ds", ["cora", "citeseer"])
@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_calc_a_hat_bit_exact(ds, mode, request):
    g = request.getfixturevalue(ds)
    ah = O.calc_a_hat(adj_of(g), mode)
    assert np.array_equal(ah.indptr, g[f"ahat_{mode}_indptr"])
    assert np.array_equal(ah.indices, g[f"ahat_{mode}_indices"])
    assert np.array_equal(ah.data, g[f"ahat_{mode}_data"])  # fp64, bit for bit


@pytest.mark.parametrize("name", ["complete5", "complete2", "path3", "isolated3", "weighted4",
                                  "selfloop3"])
@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_kat_operator_and_ppr(kat, name, mode):
    n = len(kat[f"{name}_indptr"]) - 1
    a = sp.csr_matrix((kat[f"{name}_data"], kat[f"{name}_indices"], kat[f"{name}_indptr"]),
                      shape=(n, n))
    assert np.array_equal(O.calc_a_hat(a, mode).toarray(), kat[f"{name}_ahat_{mode}_dense"])
    np.testing.assert_allclose(O.compute_ppr(a, 0.1, mode), kat[f"{name}_ppr_{mode}_a0.1"],
                               rtol=1e-12, atol=1e-14)


def test_path3_values(kat):
    """P3 sym values 0.5 / 0.40825 / 0.3333."""
    d = kat["path3_ahat_sym_dense"]
    assert d[0, 0] == pytest.approx(0.5)
    assert d[0, 1] == pytest.approx(1 / np.sqrt(6))
    assert d[1, 1] == pytest.approx(1 / 3)


@pytest.mark.parametrize("ds", ["cora", "citeseer"])
@pytest.mark.parametrize("mode,K,alpha,key", [("sym", 10, 0.1, "Z_sym_K10_a0.1"),
                                              ("sym", 20, 0.2, "Z_sym_K20_a0.2"),
                                              ("rw", 10, 0.1, "Z_rw_K10_a0.1")])
def test_propagate_matches_fixture(ds, mode, K, alpha, key, request):
    g = request.getfixturevalue(ds)
    Z = O.appnp_propagate(O.calc_a_hat(adj_of(g), mode), g["H"], K, alpha)
    np.testing.assert_allclose(Z, g[key], rtol=0, atol=1e-12)


def test_closed_form_identity(cora):
    ah = O.calc_a_hat(adj_of(cora), "sym")
    H = cora["H"]
    for K in (0, 1, 5, 10):
        np.testing.assert_allclose(O.appnp_closed_form(ah, H, K, 0.1),
                                   O.appnp_propagate(ah, H, K, 0.1), atol=1e-12)


@pytest.mark.parametrize("mode,key", [("sym", "pprH_a0.1"), ("rw", "pprH_rw_a0.1")])
def test_limit_is_compute_ppr(cora, mode, key):
    """lim_K Z_K = compute_ppr(adj, a) @ H (helpers.py:68-71)."""
    Z = O.appnp_propagate(O.calc_a_hat(adj_of(cora), mode), cora["H"], 300, 0.1)
    np.testing.assert_allclose(Z, cora[key], atol=1e-9)


def test_ppnp_forward_matches_reference(cora):
    """model.py:61-67 propagation with the fixture's encoder output."""
    X = torch.from_numpy(cora["ppnp_X"])
    W1 = torch.from_numpy(cora["ppnp_W1"])
    W2 = torch.from_numpy(cora["ppnp_W2"])
    H = (torch.relu(X @ W1) @ W2.T).double().numpy()
    ppr = O.compute_ppr(adj_of(cora), 0.1)
    out = O.ppnp_forward(ppr, H, idx=cora["ppnp_idx"])
    ref = cora["ppnp_logits"]
    assert np.abs(out - ref).max() <= 1e-5 * np.abs(ref).max()
    with pytest.raises(Exception):
        O.ppnp_forward(ppr, H)


def test_edge_mask_statistics_and_determinism():
    rows = np.repeat(np.arange(2000), 50)
    cols = np.tile(np.arange(50), 2000)
    for p in (0.1, 0.5, 0.9):
        keep = O.edge_keep_mask(rows, cols, 3, p, seed=42)
        assert abs(keep.mean() - (1 - p)) < 0.01
        assert np.array_equal(keep, O.edge_keep_mask(rows, cols, 3, p, seed=42))
    k0 = O.edge_keep_mask(rows, cols, 0, 0.5, seed=1)
    k1 = O.edge_keep_mask(rows, cols, 1, 0.5, seed=1)
    assert (k0 != k1).mean() > 0.4  # a fresh mask every iteration
    assert O.edge_keep_mask(rows, cols, 0, 0.0, seed=1).all()


def test_splitmix_scalar_vector_agree():
    xs = [0, 1, 2**63 + 5, 2**64 - 1, 123456789]
    v = O._splitmix64(np.array(xs, dtype=np.uint64))
    assert [int(a) for a in v] == [O._splitmix64(x) for x in xs]


@pytest.mark.parametrize("p", [0.0, 0.4])
def test_backward_is_adjoint(p):
    """<J H, G> == <H, J^T G> for the (masked) APPNP map."""
    adj = O.synth_graph(300, 1200, seed=3)
    ah = O.calc_a_hat(adj, "sym")
    rng = np.random.default_rng(0)
    H, G = rng.standard_normal((300, 5)), rng.standard_normal((300, 5))
    for K in (1, 3, 6):
        lhs = np.sum(O.appnp_propagate(ah, H, K, 0.1, p, 9) * G)
        rhs = np.sum(H * O.appnp_backward(ah, G, K, 0.1, p, 9))
        assert lhs == pytest.approx(rhs, rel=1e-10)


def test_torch_cpu_baseline_matches(cora):
    ah = O.calc_a_hat(adj_of(cora), "sym")
    A = O.torch_sparse_operator(ah)
    Z = O.appnp_propagate_torch_cpu(A, torch.from_numpy(cora["H"]), 10, 0.1)
    ref = cora["Z_sym_K10_a0.1"]
    assert np.abs(Z.double().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


def test_synth_graph_properties():
    a = O.synth_graph(1000, 5000, seed=1)
    assert (a != a.T).nnz == 0
    assert a.diagonal().sum() == 0
    assert np.all(a.data == 1)
    assert a.has_sorted_indices


# ---------------------------------------------------------------------------------------
# bf16 storage reference (round_bf16 / spacing_bf16 / step_exact / close_bf16_step / envelope)
# ---------------------------------------------------------------------------------------


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_round_bf16_is_torch_bfloat16_bit_for_bit():
    rng = np.random.default_rng(0)
    rand = (rng.standard_normal(200_000) * np.exp(rng.uniform(-40, 40, 200_000))).astype(np.float32)
    # exact ties: bf16 values (even and odd last bit) plus half a spacing; values that round up
    # into the next binade (mantissa all ones); +-0, +-inf, the largest finite values, denormals
    base = _bits(rng.standard_normal(4096).astype(np.float32)) & np.uint32(0xFFFF0000)
    ties = (base | np.uint32(0x8000)).view(np.float32)
    below = (base | np.uint32(0x7FFF)).view(np.float32)
    above = (base | np.uint32(0x8001)).view(np.float32)
    carry = np.array([0x3FFFFFFF, 0x3FFF8000, 0x3FFF7FFF, 0xBFFF8000, 0x7F7FFFFF, 0x7F7F8000,
                      0x7F7F7FFF, 0xFF7F8000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF,
                      0x00000000, 0x80000000, 0x7F800000, 0xFF800000], dtype=np.uint32)
    x = np.concatenate([rand, ties, below, above, carry.view(np.float32)])
    got = O.round_bf16(x)
    ref = torch.from_numpy(x).bfloat16().float().numpy()
    assert np.array_equal(_bits(got), _bits(ref))
    assert (_bits(got) & np.uint32(0xFFFF) == 0).all()
    # NaN stays NaN (quiet and signalling, either sign), as in torch
    nans = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0x7F80FFFF], dtype=np.uint32)
    out = O.round_bf16(nans.view(np.float32))
    assert np.isnan(out).all() and (_bits(out) & np.uint32(0xFFFF) == 0).all()
    assert torch.from_numpy(nans.view(np.float32).copy()).bfloat16().float().isnan().all()
    assert O.round_bf16(np.ones((3, 5), np.float32)).shape == (3, 5)


def test_spacing_bf16():
    x = np.array([1.0, 1.99, 2.0, 0.75, -3.0, 0.0, 1e-45, 2.0 ** -126, 255.0, 256.0])
    ref = np.array([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 2.0 ** -133,
                    2.0 ** -133, 2.0 ** -133, 1.0, 2.0])
    assert np.array_equal(O.spacing_bf16(x), ref)
    # it is the gap between neighbouring bf16 values
    v = O.round_bf16(np.random.default_rng(1).standard_normal(1000).astype(np.float32))
    up = ((_bits(v) + np.uint32(0x10000)).view(np.float32)).astype(np.float64)
    assert np.array_equal(np.abs(up - v.astype(np.float64)), O.spacing_bf16(v))


def _emulate_step_fp32(ah32, Z, H, alpha):
    """One forward step in fp32, every row accumulated in REVERSED entry order with separate
    multiply and add (a summation order no kernel here uses), the value before the store."""
    n, F = H.shape
    ip, ix, w = ah32.indptr, ah32.indices, ah32.data.astype(np.float32)
    deg = np.diff(ip)
    acc = np.zeros((n, F), dtype=np.float32)
    for j in range(int(deg.max())):
        rows = np.flatnonzero(deg > j)
        e = ip[rows + 1] - 1 - j
        acc[rows] = acc[rows] + (w[e][:, None] * Z[ix[e]]).astype(np.float32)
    s = np.float32(1.0) - np.float32(alpha)
    return (s * acc).astype(np.float32) + (np.float32(alpha) * H).astype(np.float32)


def test_bf16_step_bound_accepts_rounding_and_rejects_truncation():
    """The bound of close_bf16_step on an fp32 emulation of the kernel: stored with
    round-to-nearest-even it holds for every element; stored truncated it fails for about half
    of them (a truncated value is up to a whole spacing below, twice the bound)."""
    n, F, alpha = 3000, 20, 0.1
    adj = O.synth_graph(n, 15000, 3)
    ah = O.calc_a_hat(adj, "sym")
    ah32 = ah.astype(np.float32)
    rng = np.random.default_rng(5)
    Z = O.round_bf16(rng.standard_normal((n, F)).astype(np.float32))
    H = O.round_bf16(rng.standard_normal((n, F)).astype(np.float32))
    pre = _emulate_step_fp32(ah32, Z, H, alpha)
    t, delta = O.step_exact(ah32.indptr, ah32.indices, ah32.data, Z, H, alpha, 0, 0.0, 0)
    # t is the fp64 step on the fp32 operands
    s = float(np.float32(1.0) - np.float32(alpha))
    ref = (s * (ah32.astype(np.float64) @ Z.astype(np.float64))
           + float(np.float32(alpha)) * H.astype(np.float64))
    assert np.abs(t - ref).max() <= 1e-15 and (delta > 0).all() and delta.max() < 1e-4
    worst, share = O.close_bf16_step(O.round_bf16(pre), t, delta, "RNE")
    assert worst <= 1.0 and share > 0.999
    trunc = (_bits(pre) & np.uint32(0xFFFF0000)).view(np.float32)
    with pytest.raises(AssertionError):
        O.close_bf16_step(trunc, t, delta, "truncated")
    bound = 0.5 * O.spacing_bf16(np.abs(t) + delta) + delta
    ratio = np.abs(trunc.astype(np.float64) - t) / bound
    assert (ratio > 1.0).mean() > 0.4 and 1.9 < ratio.max() <= 2.0 + 1e-3
    assert (trunc == O.round_bf16(t.astype(np.float32))).mean() < 0.55
    # a wrong value in one small element fails it too
    bad = O.round_bf16(pre).copy()
    i = np.unravel_index(np.argmin(np.abs(t)), t.shape)
    bad[i] += np.float32(2.0 ** -6)
    with pytest.raises(AssertionError):
        O.close_bf16_step(bad, t, delta, "one element off")


@pytest.mark.parametrize("transposed", [False, True])
def test_step_exact_dropout_matches_masked_operator(transposed):
    """step_exact under dropout is the oracle's masked operator on the fp32 weights (mask, key
    order, fp32 scale), also for a row range keyed on global rows and for the adjoint's keys."""
    n, F, alpha, p, k, seed = 700, 5, 0.2, 0.3, 3, 11
    ah32 = O.calc_a_hat(O.synth_graph(n, 3000, 4), "rw").astype(np.float32)
    rng = np.random.default_rng(2)
    Z, H = rng.standard_normal((n, F)), rng.standard_normal((n, F))
    M = O.masked_operator(ah32.astype(np.float64), k, p, seed)  # forward keys (row, col)
    op = ah32.T.tocsr() if transposed else ah32
    op.sort_indices()
    Mop = M.T.tocsr() if transposed else M
    s, a = float(np.float32(1) - np.float32(alpha)), float(np.float32(alpha))
    t, delta = O.step_exact(op.indptr, op.indices, op.data, Z, H, alpha, k, p, seed,
                            transposed=transposed)
    ref = s * (Mop @ Z) + a * H
    # the fp32 product w32 * scale against the oracle's fp64 one: 2^-24 relative per weight
    assert np.abs(t - ref).max() <= 2.0 ** -23 * (s * (abs(Mop) @ np.abs(Z))).max()
    lo, hi = 200, 450
    sub = op[lo:hi]
    t2, d2 = O.step_exact(sub.indptr, sub.indices, sub.data, Z, H[lo:hi], alpha, k, p, seed,
                          transposed=transposed, row_lo=lo)
    assert np.array_equal(t2, t[lo:hi]) and np.array_equal(d2, delta[lo:hi])
    t3, _ = O.step_exact(op.indptr, op.indices, op.data, Z, H, alpha, k, p, seed,
                         transposed=transposed, h_weight=1.0, y_weight=alpha)
    np.testing.assert_allclose(t3, a * s * (Mop @ Z) + H, rtol=0, atol=1e-6)
    t4, _ = O.step_exact(op.indptr, op.indices, op.data, Z, None, alpha, k, p, seed,
                         transposed=transposed)
    np.testing.assert_allclose(t4, s * (Mop @ Z), rtol=0, atol=1e-6)


def test_envelope_bounds_two_faithful_chains():
    """Two fp32 emulations with different summation orders, both storing RNE bf16, iterated three
    steps from the same H: they stay within the envelope, which stays a few spacings wide."""
    n, F, alpha = 1500, 6, 0.1
    ah32 = O.calc_a_hat(O.synth_graph(n, 7000, 9), "sym").astype(np.float32)
    csr = (ah32.indptr, ah32.indices, ah32.data)
    H = O.round_bf16(np.random.default_rng(3).standard_normal((n, F)).astype(np.float32))
    za = zb = H
    E = np.zeros((n, F))
    for k in range(3):
        t, delta = O.step_exact(*csr, za, H, alpha, k, 0.0, 0)
        E = O.envelope(*csr, E, None, t, delta, alpha)
        za = O.round_bf16(t.astype(np.float32))  # forward order, one rounding
        zb = O.round_bf16(_emulate_step_fp32(ah32, zb, H, alpha))
        assert (np.abs(za.astype(np.float64) - zb) <= E).all()
        assert E.max() <= (k + 2) * 2.0 * O.spacing_bf16(np.abs(t).max())


def test_drop_threshold_follows_the_float_abi():
    """p crosses the C ABI as a float: the oracle's threshold is float32(p) * 2^24 (0.3 ->
    5033165, one more than the double 0.3 gives), matching set_drop in appnp_propagate.hip."""
    assert O.drop_threshold(0.3) == 5033165
    assert O.drop_threshold(0.5) == 1 << 23
    assert O.drop_threshold(0.0) == 0
