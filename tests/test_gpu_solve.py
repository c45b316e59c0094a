"""GPU: the exact PPNP solver (appnp_solve / ppnp_amd.solve) against the reference fixtures.

References are the reference's own dense PPR products (pprH* = compute_ppr(adj, 0.1) @ H,
helpers.py:68-71), the oracle's compute_ppr, or an fp64 replay of the Chebyshev recurrence with
the library's weights.  The bar is the project's own for the converged series, 1e-5 max|ref|
(test_gpu_parity.py::test_ppr_rows_match_compute_ppr): the fp64 replay at tol = 1e-6 sits at
<= 2.5e-6 max|ref| (tests/test_solve_abi.py), which leaves a 4x margin for fp32 summation order.
Wherever the solver must pass, the plain series with the same number of launches must miss, so
the acceleration and not a large count is what passes.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import ppnp_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALPHA = 0.1
KAT = ["complete5", "complete2", "path3", "isolated3", "weighted4", "selfloop3"]


def _pa():
    import ppnp_amd

    return ppnp_amd


def adj_of(g):
    n = int(g["n"])
    return sp.csr_matrix((g["adj_data"], g["adj_indices"], g["adj_indptr"]), shape=(n, n))


def to_np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def rel_err(Z, ref):
    err = float(np.abs(np.asarray(Z, dtype=np.float64) - ref).max())
    return err, float(np.abs(ref).max())


def replay(a_hat, H, alpha, iters):
    """The recurrence of appnp_solve in fp64 (scipy) with the library's weights."""
    from ppnp_amd.ops import solve_weights

    H = np.asarray(H, dtype=np.float64)
    prev, z = None, H
    for w in solve_weights(alpha, iters):
        t = (1.0 - alpha) * (a_hat @ z) + alpha * H
        prev, z = z, (t if prev is None else w * t + (1.0 - w) * prev)
    return z


# ---------------------------------------------------------------------------------------
# reference fixtures: narrow kernels, F = the fixture's H width
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("ds", ["cora", "citeseer"])
@pytest.mark.parametrize("mode,key", [("sym", "pprH_a0.1"), ("rw", "pprH_rw_a0.1")])
def test_solve_fixture(ds, mode, key, request):
    g = request.getfixturevalue(ds)
    pa = _pa()
    G = pa.Graph.from_scipy(adj_of(g), mode=mode, device=DEV)
    H = torch.from_numpy(g["H"]).to(DEV)
    m = pa.solve_iterations(ALPHA, 1e-6)
    assert m == 32
    ref = g[key]
    err, scale = rel_err(to_np(pa.solve(G, H, ALPHA, tol=1e-6)), ref)
    plain, _ = rel_err(to_np(pa.propagate_forward(G, H, m, ALPHA)), ref)
    print(f"{ds} {mode}: solve err {err:.3e}, plain K={m} err {plain:.3e}, bar {1e-5 * scale:.3e}")
    assert err <= 1e-5 * scale
    assert plain > 1e-5 * scale


@pytest.mark.parametrize("name", KAT)
@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_solve_known_answer_graphs(kat, name, mode):
    pa = _pa()
    n = len(kat[f"{name}_indptr"]) - 1
    G = pa.Graph.from_csr(kat[f"{name}_indptr"], kat[f"{name}_indices"], kat[f"{name}_data"], n,
                          mode=mode, device=DEV)
    H = torch.randn(n, 3, generator=torch.Generator().manual_seed(n))
    ref = kat[f"{name}_ppr_{mode}_a0.1"] @ H.double().numpy()
    err, scale = rel_err(to_np(pa.solve(G, H.to(DEV), ALPHA, tol=1e-6)), ref)
    assert err <= 1e-5 * scale, (err, scale)


# ---------------------------------------------------------------------------------------
# kernel variants: a latency-regime graph with heavy rows and a hub row
# ---------------------------------------------------------------------------------------

WIDTHS = [1, 3, 7, 16, 33, 64, 100, 130]


@pytest.fixture(scope="module")
def hub(cora):
    """Cora-ML plus one node joined to 600 others: a hub row (601 > kHubRow = 512 entries of
    A_hat) and heavy rows (> kHeavyRow = 32).  (adj, a_hat fp64, Pi fp64, H fp64 [n, 130])."""
    a = adj_of(cora).tolil()
    n = a.shape[0] + 1
    b = sp.lil_matrix((n, n), dtype=np.float32)
    b[:n - 1, :n - 1] = a
    nb = np.random.default_rng(7).choice(n - 1, 600, replace=False)
    b[n - 1, nb] = 1.0
    b[nb, n - 1] = 1.0
    adj = b.tocsr()
    adj.sort_indices()
    a_hat = O.calc_a_hat(adj, "sym")
    lens = np.diff(a_hat.indptr)
    assert lens.max() > 512 and (lens > 32).sum() > 1
    pi = O.compute_ppr(adj, ALPHA, "sym")
    H = np.random.default_rng(11).standard_normal((n, max(WIDTHS)))
    return adj, a_hat, pi, H.astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def hub_graph(hub):
    return _pa().Graph.from_scipy(hub[0], mode="sym", device=DEV)


def _operand(h, layout):
    """H [n, f] on the device, an output buffer in the named memory layout, and the padding
    columns of that buffer (NaN; None where the layout has none)."""
    n, f = h.shape
    src = torch.from_numpy(h.astype(np.float32))
    if layout == "contiguous":
        return src.to(DEV), None, None
    if layout == "ld104":  # padded rows of 104 floats, 16-B vectors
        Hd = torch.zeros(n, 104, device=DEV)[:, :f]
        Hd.copy_(src)
        buf = torch.full((n, 104), float("nan"), device=DEV)
        return Hd, buf[:, :f], buf[:, f:]
    # base pointers 4 bytes past a 16-B boundary: only V = 1 is aligned
    Hd = torch.zeros(n * f + 1, device=DEV)[1:].view(n, f)
    Hd.copy_(src)
    return Hd, torch.full((n * f + 1,), float("nan"), device=DEV)[1:].view(n, f), None


# F = 101, 98, 99 in rows of 104 floats: the hub graph's heavy rows keep V = 4 in the latency
# regime, so the Chebyshev epilogue runs its vector tails of 1, 2 and 3 elements
CASES = ([(f, "contiguous") for f in WIDTHS] + [(100, "ld104"), (100, "offset4")]
         + [(101, "ld104"), (98, "ld104"), (99, "ld104")])


@pytest.mark.parametrize("f,layout", CASES)
def test_solve_kernel_variants(hub, hub_graph, f, layout):
    pa = _pa()
    _, _, pi, H = hub
    h = H[:, :f]
    ref = pi @ h
    m = pa.solve_iterations(ALPHA, 1e-6)
    Hd, out, pad = _operand(h, layout)
    if layout == "offset4":
        assert Hd.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    Z = pa.solve_forward(hub_graph, Hd, m, ALPHA, out=out)
    if pad is not None:
        assert bool(torch.isnan(pad).all())  # the output's padding is not written
    err, scale = rel_err(to_np(Z), ref)
    plain, _ = rel_err(to_np(pa.propagate_forward(hub_graph, Hd, m, ALPHA)), ref)
    print(f"F={f} {layout}: solve err {err:.3e}, plain err {plain:.3e}, bar {1e-5 * scale:.3e}")
    assert err <= 1e-5 * scale
    assert plain > 1e-5 * scale
    assert torch.equal(Hd.cpu(), torch.from_numpy(h.astype(np.float32)))  # H is read only


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("f", [7, 100])
def test_solve_first_steps_match_replay(hub, hub_graph, f, iters):
    """Exactly `iters` steps: step 1 is the plain step, step 2 reads H as Z_{k-1}, step 3 reads
    Z_{k-1} from the buffer it overwrites."""
    pa = _pa()
    _, a_hat, _, H = hub
    h = H[:, :f]
    ref = replay(a_hat, h, ALPHA, iters)
    Z = pa.solve_forward(hub_graph, torch.from_numpy(h.astype(np.float32)).to(DEV), iters, ALPHA)
    err, scale = rel_err(to_np(Z), ref)
    assert err <= 1e-6 * scale, (err, scale)


@pytest.mark.parametrize("iters", [4, 5])
def test_solve_both_buffer_rotations_match_replay(hub, hub_graph, iters):
    """An even and an odd count past 3: the last step lands in Z from either workspace buffer."""
    pa = _pa()
    _, a_hat, _, H = hub
    h = H[:, :33]
    ref = replay(a_hat, h, ALPHA, iters)
    Z = pa.solve_forward(hub_graph, torch.from_numpy(h.astype(np.float32)).to(DEV), iters, ALPHA)
    err, scale = rel_err(to_np(Z), ref)
    assert err <= 1e-6 * scale, (err, scale)


# ---------------------------------------------------------------------------------------
# bandwidth regime (> 2^16 rows), on a graph that has the source-blocked copy
# ---------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def big():
    """uniform_graph(70 000, 1 000 000) with the source-blocked copy of F = 100, H [n, 128] and
    the fp64 replay of 32 steps for all 128 columns.  The solve is linear and column-separable,
    so its first 100 columns are the reference of F = 100, and so that the replay takes 2 s of
    scipy instead of 15, H = B R with B [n, 16] and R [16, 128]: the replay runs on B and the
    reference is replay(B) R.  The device gets fl32(B R), which differs from B R by at most
    2^-24 |B R| per element; the solve's operator is a polynomial in A_hat with row sums near 1,
    so that moves the reference by about 1e-7 max|ref|, a hundredth of the bar."""
    from ppnp_amd.synth import uniform_graph

    pa = _pa()
    n = 70_000
    ip, ix = uniform_graph(n, 1_000_000, 5, device=DEV)
    G = pa.Graph.from_csr(ip, ix, None, n, mode="sym", device=DEV, features=100)
    assert G.source_block_layout() is not None and G.remainder_cols(100) == 4
    rp, col, val, _ = G.csr()
    a_hat = sp.csr_matrix((val.cpu().numpy().astype(np.float64), col.cpu().numpy(),
                           rp.cpu().numpy()), shape=(n, n))
    rng = np.random.default_rng(9)
    B, R = rng.standard_normal((n, 16)), rng.standard_normal((16, 128)) / 4
    m = pa.solve_iterations(ALPHA, 1e-6)
    return G, torch.from_numpy((B @ R).astype(np.float32)), m, replay(a_hat, B, ALPHA, m) @ R


@pytest.mark.parametrize("f", [100, 128])
def test_solve_bandwidth_regime_gathers_whole_rows(big, f):
    pa = _pa()
    G, H, m, ref = big
    Hd = H[:, :f].contiguous().to(DEV)
    before = G.source_block_layout()["launches"]
    Z = pa.solve(G, Hd, ALPHA, tol=1e-6)
    torch.cuda.synchronize()
    assert G.source_block_layout()["launches"] == before  # no remainder pass
    err, scale = rel_err(to_np(Z), ref[:, :f])
    print(f"F={f}: err {err:.3e}, bar {1e-5 * scale:.3e}")
    assert err <= 1e-5 * scale


# ---------------------------------------------------------------------------------------
# backward, errors
# ---------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def cora_pi(cora):
    adj = adj_of(cora)
    return {mode: O.compute_ppr(adj, ALPHA, mode) for mode in ("sym", "rw")}


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_solve_backward_is_the_transposed_operator(cora, cora_pi, mode):
    pa = _pa()
    G = pa.Graph.from_scipy(adj_of(cora), mode=mode, device=DEV, transpose=True)
    H = torch.from_numpy(cora["H"]).to(DEV).requires_grad_(True)
    dZ = torch.randn(H.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    Z = pa.solve(G, H, ALPHA, tol=1e-6)
    (dH,) = torch.autograd.grad(Z, H, dZ)
    ref = cora_pi[mode].T @ to_np(dZ)
    err, scale = rel_err(to_np(dH), ref)
    assert err <= 1e-5 * scale, (err, scale)


def test_solve_backward_rw_needs_the_transpose(cora):
    pa = _pa()
    G = pa.Graph.from_scipy(adj_of(cora), mode="rw", device=DEV)
    H = torch.from_numpy(cora["H"]).to(DEV).requires_grad_(True)
    Z = pa.solve(G, H, ALPHA, tol=1e-6)
    with pytest.raises(pa._lib.AppnpError) as e:
        torch.autograd.grad(Z, H, torch.ones_like(Z))
    assert e.value.code == pa._lib.APPNP_ENOTSUP


def test_solve_rejects_directed_graphs_and_bf16(cora):
    pa = _pa()
    a = sp.csr_matrix(np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float32))
    G = pa.Graph.from_scipy(a, device=DEV, transpose=True)
    assert not G.symmetric
    with pytest.raises(pa._lib.AppnpError) as e:
        pa.solve(G, torch.ones(3, 4, device=DEV))
    assert e.value.code == pa._lib.APPNP_ENOTSUP
    G = pa.Graph.from_scipy(adj_of(cora), device=DEV)
    with pytest.raises(pa._lib.AppnpError) as e:
        pa.solve_forward(G, torch.ones(G.n, 8, device=DEV, dtype=torch.bfloat16), 8, ALPHA)
    assert e.value.code == pa._lib.APPNP_ENOTSUP
    H = torch.ones(G.n, 8, device=DEV)
    with pytest.raises(pa._lib.AppnpError) as e:
        pa.solve_forward(G, H, 8, ALPHA, out=H)
    assert e.value.code == pa._lib.APPNP_EINVAL


# ---------------------------------------------------------------------------------------
# model, PPR rows, plan
# ---------------------------------------------------------------------------------------


@pytest.fixture()
def cora_fresh():
    """The Cora-ML fixture read from disk again: the session's copy of ``ppnp_X`` is thresholded
    in place by test_gpu_parity.py::test_model_sparse_input_matches_dense, which runs earlier."""
    import os

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for part in ("", "_ppnp"):
        out.update(np.load(os.path.join(golden, f"cora_ml{part}.npz"), allow_pickle=False))
    return out


def test_model_exact_reproduces_ppnp_logits(cora_fresh):
    """APPNP(exact=True) is the reference's PPNP (model.py:41-67) without K = 200."""
    cora = cora_fresh
    pa = _pa()
    C = int(cora["n_classes"])
    X = torch.from_numpy(cora["ppnp_X"]).to(DEV)
    model = pa.APPNP(n_features=X.shape[1], n_classes=C, adj=adj_of(cora), exact=True,
                     tol=1e-6).to(DEV).eval()
    model.encoder[1].weight.data.copy_(torch.from_numpy(cora["ppnp_W1"]))
    model.encoder[4].weight.data.copy_(torch.from_numpy(cora["ppnp_W2"]))
    idx = torch.from_numpy(cora["ppnp_idx"]).to(DEV)
    with torch.no_grad():
        out = model(X, idx).cpu().numpy()
    ref = cora["ppnp_logits"]
    assert np.abs(out - ref).max() <= 1e-4 * np.abs(ref).max()
    # the plain model at K = 10 is a different function
    plain = pa.APPNP(n_features=X.shape[1], n_classes=C, adj=adj_of(cora)).to(DEV).eval()
    plain.load_state_dict(model.state_dict())
    with torch.no_grad():
        out10 = plain(X, idx).cpu().numpy()
    assert np.abs(out10 - ref).max() > 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_ppr_rows_with_tol_match_compute_ppr(cora, cora_pi, mode):
    from ppnp_amd.ppr import ppr_rows

    pa = _pa()
    G = pa.Graph.from_scipy(adj_of(cora), mode=mode, device=DEV)
    idx = torch.tensor([0, 5, 17, 2809, 1400, 77])
    rows = ppr_rows(G, idx, alpha=ALPHA, tol=1e-6).cpu().numpy()
    ref = cora_pi[mode][idx.numpy()]
    assert np.abs(rows - ref).max() <= 1e-5 * np.abs(ref).max()
    m = pa.solve_iterations(ALPHA, 1e-6)
    plain = ppr_rows(G, idx, K=m, alpha=ALPHA).cpu().numpy()
    assert np.abs(plain - ref).max() > 1e-5 * np.abs(ref).max()


def test_solve_plan_replays_the_direct_call_bit_for_bit(cora):
    pa = _pa()
    G = pa.Graph.from_scipy(adj_of(cora), device=DEV)
    H = torch.from_numpy(cora["H"]).to(DEV)
    direct = pa.solve(G, H, ALPHA, tol=1e-6)
    plan = pa.SolvePlan(G, H.clone(), ALPHA, tol=1e-6)
    assert plan.iters == 32
    assert torch.equal(plan(), direct)
    plan.H.mul_(2.0)  # refill in place, replay
    assert torch.equal(plan(), pa.solve(G, plan.H, ALPHA, tol=1e-6))
    plan.close()
