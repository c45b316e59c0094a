"""GPU: polynomial propagation with device coefficients (appnp_poly / ppnp_amd.poly, GPRGNN).

Reference: tests/poly_ref.py, fp64 scipy on the oracle's calc_a_hat.  Bars: Z and dH take the
project's fp32 bar, 1e-5 max|ref| + 1e-6.  d gamma_k is a dot product of n F terms, so its
error is measured in S_k = sum |G_k o H|, the sum of the absolute terms: |d gamma_k - ref_k| <=
1e-5 S_k + 1e-6.  A CPU emulation of the kernel's arithmetic (fp32 SpMM, fp32 row partials, fp64
sum) sits at 2.7e-8 .. 6.7e-8 S_k on Cora-ML, so the bar leaves about 150x for the GPU's
summation order.  With H standard normal and dZ = H + 0.5 noise, neighbouring d gamma differ by
far more than the bar (asserted below: > 100 bars), so an off-by-one in k cannot pass.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import poly_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KAT = ["complete5", "complete2", "path3", "isolated3", "weighted4", "selfloop3"]
WIDTHS = [1, 3, 7, 16, 33, 64, 100, 130, 260]
WORST = {"dcoef": 0.0}  # the worst |d gamma - ref| / S seen in this session, printed per test


def _pa():
    import ppnp_amd

    return ppnp_amd


def adj_of(g):
    n = int(g["n"])
    return sp.csr_matrix((g["adj_data"], g["adj_indices"], g["adj_indptr"]), shape=(n, n))


def to_np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def check_dense(name, got, ref):
    err = float(np.abs(to_np(got) - ref).max())
    bar = 1e-5 * float(np.abs(ref).max()) + 1e-6
    print(f"  {name}: err {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (name, err, bar)


def check_dcoef(got, ref, S, tag=""):
    got = to_np(got)
    assert got.shape == ref.shape
    bar = 1e-5 * S + 1e-6
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(S, 1e-30)).max())
    WORST["dcoef"] = max(WORST["dcoef"], ratio)
    print(f"  dcoef {tag}: worst |err| / S_k = {ratio:.3e} (bar 1e-5; session worst "
          f"{WORST['dcoef']:.3e})")
    assert (err <= bar).all(), (tag, err, bar)


def assert_discriminates(ref, S):
    """Neighbouring d gamma lie more than 100 bars apart: a k off by one cannot pass."""
    bar = 1e-5 * S + 1e-6
    gap = np.abs(np.diff(ref))
    assert (gap > 100 * np.maximum(bar[:-1], bar[1:])).all(), (gap, bar)


class Ref:
    """The fp64 reference of one (graph, H, dZ, coef) at its full width, cut to the first f
    columns on demand: Z and dH are column-separable, d gamma_k and S_k are sums over columns,
    kept per column and accumulated."""

    def __init__(self, a, H, dZ, coef):
        self.H, self.dZ, self.coef = H, dZ, np.asarray(coef, dtype=np.float64)
        self.Z = poly_ref.forward(a, H, coef)
        at = a.T.tocsr()
        g = dZ.astype(np.float64)
        self.dH = self.coef[0] * g
        cols, abss = [(g * H).sum(axis=0)], [np.abs(g * H).sum(axis=0)]
        for c in self.coef[1:]:
            g = at @ g
            self.dH = self.dH + c * g
            cols.append((g * H).sum(axis=0))
            abss.append(np.abs(g * H).sum(axis=0))
        self.dcoef_cols, self.S_cols = np.array(cols), np.array(abss)
        for x in (self.Z, self.dH, self.dcoef_cols, self.S_cols):
            x.setflags(write=False)

    def at(self, f):
        return (self.Z[:, :f], self.dH[:, :f], self.dcoef_cols[:, :f].sum(axis=1),
                self.S_cols[:, :f].sum(axis=1))


def inputs(n, f, seed):
    """H standard normal (float32 values), dZ = H + 0.5 noise."""
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((n, f)).astype(np.float32).astype(np.float64)
    dZ = (H + 0.5 * rng.standard_normal((n, f))).astype(np.float32).astype(np.float64)
    return H, dZ


def run(G, Hd, dZd, coefd):
    from ppnp_amd import ops

    Z = ops.poly_forward(G, Hd, coefd)
    dH, dcoef = ops.poly_backward(G, dZd, Hd, coefd)
    return Z, dH, dcoef


def check_all(G, Hd, dZd, coef, ref_at, tag):
    Z, dH, dcoef = run(G, Hd, dZd, dev(coef))
    rZ, rdH, rdc, S = ref_at
    print(tag)
    check_dense("Z", Z, rZ)
    check_dense("dH", dH, rdH)
    check_dcoef(dcoef, rdc, S, tag)
    return Z, dH, dcoef


# ---------------------------------------------------------------------------------------
# 1. known-answer graphs
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", KAT)
@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_poly_known_answer_graphs(kat, name, mode):
    pa = _pa()
    ip, ix, dv = kat[f"{name}_indptr"], kat[f"{name}_indices"], kat[f"{name}_data"]
    n = len(ip) - 1
    G = pa.Graph.from_csr(ip, ix, dv, n, mode=mode, device=DEV, transpose=(mode == "rw"))
    a = poly_ref.a_hat(sp.csr_matrix((dv, ix, ip), shape=(n, n)), mode)
    H, dZ = inputs(n, 3, n)
    rng = np.random.default_rng(17)
    for K in (4, 0, 1):
        coef = rng.standard_normal(K + 1).astype(np.float32).astype(np.float64)
        if K == 4:
            coef[1], coef[2] = -abs(coef[1]) - 0.25, 0.0  # a negative and a zero coefficient
        ref = Ref(a, H, dZ, coef)
        check_all(G, dev(H), dev(dZ), coef, ref.at(3), f"{name} {mode} K={K}")


# ---------------------------------------------------------------------------------------
# 2. the PPR coefficients are appnp_propagate
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_poly_with_ppr_coefficients_is_propagate(cora, mode):
    pa = _pa()
    K, alpha = 10, 0.1
    G = pa.Graph.from_scipy(adj_of(cora), mode=mode, device=DEV, transpose=True)
    a = poly_ref.a_hat(adj_of(cora), mode)
    H = cora["H"].astype(np.float64)
    dZ = np.random.default_rng(1).standard_normal(H.shape).astype(np.float32).astype(np.float64)
    coef = pa.ppr_coefficients(K, alpha).double().numpy()
    ref = Ref(a, H, dZ, coef)
    Z, dH, _ = check_all(G, dev(H), dev(dZ), coef, ref.at(H.shape[1]), f"cora {mode} ppr")
    print("against propagate_forward / propagate_backward")
    check_dense("Z", Z, to_np(pa.propagate_forward(G, dev(H), K, alpha)))
    check_dense("dH", dH, to_np(pa.propagate_backward(G, dev(dZ), K, alpha)))


# ---------------------------------------------------------------------------------------
# 3. kernel variants: a latency-regime graph with heavy rows and a hub row
# ---------------------------------------------------------------------------------------

COEF3 = np.array([0.5, -0.75, 0.0, 1.25])  # K = 3


@pytest.fixture(scope="module")
def hub(cora):
    """Cora-ML plus one node joined to 600 others: a hub row (601 > kHubRow = 512 entries of
    A_hat) and heavy rows (> kHeavyRow = 32).  (Graph, reference at 260 columns)."""
    a = adj_of(cora).tolil()
    n = a.shape[0] + 1
    b = sp.lil_matrix((n, n), dtype=np.float32)
    b[:n - 1, :n - 1] = a
    nb = np.random.default_rng(7).choice(n - 1, 600, replace=False)
    b[n - 1, nb] = 1.0
    b[nb, n - 1] = 1.0
    adj = b.tocsr()
    adj.sort_indices()
    a_hat = poly_ref.a_hat(adj, "sym")
    lens = np.diff(a_hat.indptr)
    assert lens.max() > 512 and (lens > 32).sum() > 1
    H, dZ = inputs(n, max(WIDTHS), 11)
    return _pa().Graph.from_scipy(adj, mode="sym", device=DEV), Ref(a_hat, H, dZ, COEF3)


@pytest.mark.parametrize("f", WIDTHS)
def test_poly_kernel_variants(hub, f):
    G, ref = hub
    rZ, rdH, rdc, S = ref.at(f)
    assert_discriminates(rdc, S)
    check_all(G, dev(ref.H[:, :f]), dev(ref.dZ[:, :f]), COEF3, (rZ, rdH, rdc, S), f"hub F={f}")


def _padded(x, ld, offset):
    """x [n, f] on the device in rows of ld floats starting `offset` floats past an aligned base;
    the padding is NaN, so a lane that lets it into a sum shows."""
    n, f = x.shape
    buf = torch.full((n * ld + offset,), float("nan"), device=DEV)
    view = buf[offset:].view(n, ld)[:, :f]
    view.copy_(torch.from_numpy(x.astype(np.float32)))
    return view


@pytest.mark.parametrize("f,ld,offset", [(100, 103, 1),   # nothing aligned: V = 1
                                         (101, 104, 0), (98, 104, 0), (99, 104, 0)])  # V = 4 tails
def test_poly_padded_operands(hub, f, ld, offset):
    """A leading dimension above F.  (103, offset 1): only V = 1 is aligned.  Rows of 104 floats:
    the hub graph's heavy rows keep V = 4, so the last lane of a row holds 1, 2 or 3 valid
    columns and must keep the NaN padding of H and dZ out of the dot."""
    from ppnp_amd import ops

    G, ref = hub
    Hd, dZd = _padded(ref.H[:, :f], ld, offset), _padded(ref.dZ[:, :f], ld, offset)
    if offset:
        assert Hd.data_ptr() % 16 == 4
    out = _padded(np.zeros((G.n, f)), ld, offset)
    coef = dev(COEF3)
    rZ, rdH, rdc, S = ref.at(f)
    Z = ops.poly_forward(G, Hd, coef, out=out)
    dH, dcoef = ops.poly_backward(G, dZd, Hd, coef)
    print(f"hub F={f} ld={ld} offset={offset}")
    check_dense("Z", Z, rZ)
    check_dense("dH", dH, rdH)
    check_dcoef(dcoef, rdc, S, f"F={f} ld={ld}")
    pad = out.as_strided((G.n - 1, ld - f), (ld, 1), out.storage_offset() + f)
    assert bool(torch.isnan(pad).all())  # the output's padding is not written


@pytest.fixture(scope="module")
def light():
    """A cora-sized graph without heavy rows (every row of A_hat <= 32 entries): the narrow
    kernels run every row, the dot included."""
    from ppnp_amd.synth import uniform_graph

    pa = _pa()
    n = 3000
    ip, ix = uniform_graph(n, 9000, 3, device=DEV)
    G = pa.Graph.from_csr(ip, ix, None, n, mode="sym", device=DEV)
    adj = sp.csr_matrix((np.ones(ix.numel(), dtype=np.float32), ix.cpu().numpy(),
                         ip.cpu().numpy()), shape=(n, n))
    a_hat = poly_ref.a_hat(adj, "sym")
    assert np.diff(a_hat.indptr).max() <= 32
    H, dZ = inputs(n, 8, 5)
    return G, Ref(a_hat, H, dZ, COEF3)


@pytest.mark.parametrize("f", [1, 3, 7, 8])
def test_poly_narrow_kernels_take_the_dot(light, f):
    G, ref = light
    check_all(G, dev(ref.H[:, :f]), dev(ref.dZ[:, :f]), COEF3, ref.at(f), f"light F={f}")


# ---------------------------------------------------------------------------------------
# 4. reproducibility
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("which,f", [("hub", 100), ("hub", 260), ("light", 7)])
def test_poly_is_bitwise_reproducible(hub, light, which, f):
    G, ref = hub if which == "hub" else light
    f = min(f, ref.H.shape[1])
    Hd, dZd, coef = dev(ref.H[:, :f]), dev(ref.dZ[:, :f]), dev(COEF3)
    first = run(G, Hd, dZd, coef)
    torch.cuda.synchronize()
    second = run(G, Hd, dZd, coef)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------
# 5. autograd, model
# ---------------------------------------------------------------------------------------


def test_poly_autograd_for_H_and_coef(hub):
    pa = _pa()
    G, ref = hub
    f = 16
    rZ, rdH, rdc, S = ref.at(f)
    H = dev(ref.H[:, :f]).requires_grad_(True)
    coef = dev(COEF3).requires_grad_(True)
    W = dev(ref.dZ[:, :f])
    loss = (pa.poly(G, H, coef) * W).sum()
    gH, gc = torch.autograd.grad(loss, (H, coef))
    check_dense("dH", gH, rdH)
    check_dcoef(gc, rdc, S, "autograd")
    # H alone: no dot is computed, the same dH
    (gH2,) = torch.autograd.grad((pa.poly(G, H, coef.detach()) * W).sum(), (H,))
    assert torch.equal(gH, gH2)


@pytest.fixture()
def cora_fresh():
    """The Cora-ML fixture read from disk again (another test thresholds ``ppnp_X`` in place)."""
    import os

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for part in ("", "_ppnp"):
        out.update(np.load(os.path.join(golden, f"cora_ml{part}.npz"), allow_pickle=False))
    return out


def _models(cora, **kw):
    pa = _pa()
    C = int(cora["n_classes"])
    X = torch.from_numpy(cora["ppnp_X"]).to(DEV)
    adj = adj_of(cora)
    gpr = pa.GPRGNN(n_features=X.shape[1], n_classes=C, adj=adj, K=10, alpha=0.1, **kw).to(DEV)
    plain = pa.APPNP(n_features=X.shape[1], n_classes=C, adj=adj, K=10, alpha=0.1).to(DEV)
    for m in (gpr, plain):
        m.encoder[1].weight.data.copy_(torch.from_numpy(cora["ppnp_W1"]))
        m.encoder[4].weight.data.copy_(torch.from_numpy(cora["ppnp_W2"]))
    return gpr, plain, X, torch.from_numpy(cora["ppnp_idx"]).to(DEV)


def test_gprgnn_with_fixed_ppr_coefficients_is_appnp(cora_fresh):
    gpr, plain, X, idx = _models(cora_fresh, init="ppr", learn_coef=False)
    gpr.eval(), plain.eval()
    with torch.no_grad():
        out, ref = gpr(X, idx), to_np(plain(X, idx))
    check_dense("logits", out, ref)


def test_gprgnn_optimiser_step_moves_coef(cora_fresh):
    gpr, _, X, idx = _models(cora_fresh, init="ppr", learn_coef=True)
    before = gpr.coef.detach().clone()
    opt = torch.optim.SGD(gpr.parameters(), lr=0.1)
    gpr.train()
    y = torch.arange(idx.numel(), device=DEV) % gpr.n_classes
    loss = torch.nn.functional.cross_entropy(gpr(X, idx), y)
    opt.zero_grad()
    loss.backward()
    assert gpr.coef.grad is not None and bool(torch.isfinite(gpr.coef.grad).all())
    assert float(gpr.coef.grad.abs().max()) > 0
    opt.step()
    assert not torch.equal(gpr.coef.detach(), before)


# ---------------------------------------------------------------------------------------
# 6. stream order: the coefficients are read on the device
# ---------------------------------------------------------------------------------------


def test_poly_graph_capture_replays_after_refill(light):
    """Forward and backward are linear chains of launches on one stream.  Captured once, a
    replay follows H, dZ and coef as they are then: refilled in place, the results equal the
    eager ones bit for bit, so no coefficient was baked in on the host."""
    G, ref = light
    f = 7
    Hd, dZd, coef = dev(ref.H[:, :f]), dev(ref.dZ[:, :f]), dev(COEF3)
    run(G, Hd, dZd, coef)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Z, dH, dcoef = run(G, Hd, dZd, coef)
    fills = [(ref.H[:, :f], ref.dZ[:, :f], COEF3),
             (ref.dZ[:, :f] * 0.5, ref.H[:, :f] + 1.0, np.array([-1.0, 0.25, 2.0, -0.5]))]
    for h, dz, c in fills:
        Hd.copy_(dev(h)), dZd.copy_(dev(dz)), coef.copy_(dev(c))
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (Z, dH, dcoef)]
        eager = run(G, Hd, dZd, coef)
        for a, b in zip(got, eager):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the two fills gave different results: the replay did follow the refill
    assert not torch.equal(got[2], dev(ref.at(f)[2]))


# ---------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------


def test_poly_refusals(cora):
    from ppnp_amd import ops

    pa = _pa()
    L = pa._lib
    adj = adj_of(cora)
    G = pa.Graph.from_scipy(adj, device=DEV)
    coef = dev(COEF3)
    Hb = torch.ones(G.n, 8, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(L.AppnpError) as e:
        ops.poly_forward(G, Hb, coef)
    assert e.value.code == L.APPNP_ENOTSUP
    with pytest.raises(L.AppnpError) as e:
        ops.poly_backward(G, Hb, Hb, coef)
    assert e.value.code == L.APPNP_ENOTSUP
    H = torch.ones(G.n, 8, device=DEV)
    with pytest.raises(L.AppnpError) as e:
        ops.poly_forward(G, H, coef, out=H)
    assert e.value.code == L.APPNP_EINVAL
    # rw, and a directed graph, without the transpose: the forward runs, the backward cannot
    d = sp.csr_matrix(np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float32))
    for g in (pa.Graph.from_scipy(adj, mode="rw", device=DEV),
              pa.Graph.from_scipy(d, mode="sym", device=DEV)):
        h = torch.ones(g.n, 4, device=DEV)
        Z = ops.poly_forward(g, h, coef)
        assert bool(torch.isfinite(Z).all())
        for need in (True, False):
            with pytest.raises(L.AppnpError) as e:
                ops.poly_backward(g, h, h, coef, need_dcoef=need)
            assert e.value.code == L.APPNP_ENOTSUP
    # a row partition
    part = pa.Graph.from_scipy(adj, device=DEV, row_lo=0, row_hi=G.n // 2)
    with pytest.raises(L.AppnpError) as e:
        ops.poly_forward(part, H, coef)
    assert e.value.code == L.APPNP_EINVAL
    with pytest.raises(L.AppnpError) as e:
        ops.poly_backward(part, H, torch.zeros_like(H), coef)
    assert e.value.code == L.APPNP_EINVAL


def test_poly_directed_graph_forward_and_backward():
    """A directed graph with the transpose: the forward on A_hat, the backward on A_hat^T."""
    pa = _pa()
    rng = np.random.default_rng(2)
    n = 200
    d = sp.random(n, n, density=0.03, random_state=4, format="csr", dtype=np.float32)
    d.data[:] = 1.0
    d.setdiag(0)
    d.eliminate_zeros()
    d.sort_indices()
    coef = rng.standard_normal(5)
    coef = coef.astype(np.float32).astype(np.float64)
    H, dZ = inputs(n, 5, 8)
    for mode in ("sym", "rw"):
        G = pa.Graph.from_scipy(d, mode=mode, device=DEV, transpose=True)
        assert not G.symmetric
        ref = Ref(poly_ref.a_hat(d, mode), H, dZ, coef)
        check_all(G, dev(H), dev(dZ), coef, ref.at(5), f"directed {mode}")
