"""GPU: sparse top-k PPR rows (ppr.topk_rows / sparsified_ppr / SparsePPR) on Cora-ML, and the
minibatch protocol of batch-main.py:104-169 on them.

Membership bound.  The device columns differ from the fp64 oracle's by at most E in the sup norm
(E is measured in the test, from ``ppr_columns`` / ``dense_ppr``, code that does not use the
selection).  Order statistics are 1-Lipschitz in the sup norm, so the device's k-th value lies
within E of the reference's, and a reference entry more than 2E above (below) its row's k-th
value must be present (absent).  Entries within 2E of the threshold are left out of the
membership check; two conditions keep that from hiding a failure: 2E <= 4e-6, and the left-out
share of the rows * k reference entries is <= 6 % (the reference alone gives 3.8-4.5 % at k = 32
and 1.3-3.7 % at k = 128 for margins 2e-7 ... 4e-6: clusters of structurally equal PPR values).
The margin is the unscaled 2E in both modes (for rw that is the stricter reading); kept values
must match within E, for rw scaled by the row's D_max / d_i (Pi[i, j] = D_j Pi[j, i] / d_i).
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import ppnp_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALPHA = 0.1
TOL = 1e-7


def _pa():
    import ppnp_amd

    return ppnp_amd


@pytest.fixture(scope="module")
def adj(cora):
    n = int(cora["n"])
    return sp.csr_matrix((cora["adj_data"], cora["adj_indices"], cora["adj_indptr"]), shape=(n, n))


@pytest.fixture(scope="module")
def oracle_ppr(adj):
    """The fp64 oracle's Pi per mode, computed once and left unchanged."""
    out = {m: O.compute_ppr(adj, ALPHA, m) for m in ("sym", "rw")}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def graphs(adj):
    pa = _pa()
    return {m: pa.Graph.from_scipy(adj, mode=m, device=DEV) for m in ("sym", "rw")}


def dense_mask(P):
    """(stored-entry mask, values) of a SparsePPR as dense numpy arrays."""
    ip = P.indptr.cpu().numpy().astype(np.int64)
    ix = P.indices.cpu().numpy().astype(np.int64)
    row = np.repeat(np.arange(P.shape[0]), np.diff(ip))
    mask = np.zeros(P.shape, dtype=bool)
    vals = np.zeros(P.shape, dtype=np.float64)
    mask[row, ix] = True
    vals[row, ix] = P.data.cpu().numpy()
    assert mask.sum() == len(ix), "duplicate entries"
    return mask, vals


def check_membership(mask, vals, R, kth, E, k, val_bound, tag):
    """mask / vals: the device selection [rows, N]; R: reference rows; kth [rows, 1]."""
    margin = 2.0 * E
    must = R > kth + margin
    mustnot = R < kth - margin
    left_out = ~(must | mustnot)
    share = left_out.sum() / (R.shape[0] * k)
    missing = int((must & ~mask).sum())
    extra = int((mustnot & mask).sum())
    verr = float((np.abs(vals - R)[mask] / np.broadcast_to(val_bound, R.shape)[mask]).max())
    print(f"{tag}: E {E:.3e}, left-out share {share:.4f}, missing {missing}, extra {extra}, "
          f"value error / bound {verr:.3f}")
    assert margin <= 4e-6
    assert share <= 0.06
    assert missing == 0 and extra == 0
    assert verr <= 1.0


@pytest.mark.parametrize("mode", ["sym", "rw"])
@pytest.mark.parametrize("k", [32, 128])
def test_topk_rows_against_the_oracle(adj, oracle_ppr, graphs, mode, k):
    from ppnp_amd.ppr import ppr_columns, topk_rows

    G, Pi = graphs[mode], oracle_ppr[mode]
    n = G.n
    idx = np.sort(np.random.default_rng(17).choice(n, 256, replace=False))
    tidx = torch.from_numpy(idx).to(DEV)
    cols = ppr_columns(G, tidx, alpha=ALPHA, tol=TOL).cpu().numpy()
    E = float(np.abs(cols.astype(np.float64) - Pi[:, idx].astype(np.float32)).max())
    P = topk_rows(G, tidx, k, alpha=ALPHA, tol=TOL)
    assert P.shape == (256, n)
    assert np.array_equal(P.indptr.cpu().numpy(), k * np.arange(257))
    ix = P.indices.cpu().numpy().reshape(256, k)
    assert (np.diff(ix, axis=1) > 0).all(), "columns not strictly increasing"
    mask, vals = dense_mask(P)
    R = Pi[idx, :]
    kth = -np.partition(-R, k - 1, axis=1)[:, k - 1:k]
    if mode == "sym":
        bound = np.full((256, 1), E)
    else:
        deg = np.asarray(adj.sum(axis=1)).ravel() + 1.0
        bound = (E * deg.max() / deg[idx])[:, None]
    check_membership(mask, vals, R, kth, E, k, bound, f"topk_rows {mode} k={k}")


def test_sparsified_ppr_against_the_literal_quirk(oracle_ppr, graphs):
    """batch-main.py:115-116 on the oracle's Pi: entry (i, j) survives iff it is >= the k-th
    largest value of row j.  The sparse build keeps exactly k per column."""
    from ppnp_amd.ppr import dense_ppr, sparsified_ppr

    k = 32
    G, Pi = graphs["sym"], oracle_ppr["sym"]
    n = G.n
    E = float(np.abs(dense_ppr(G, alpha=ALPHA, tol=TOL).cpu().numpy().astype(np.float64)
                     - Pi.astype(np.float32)).max())
    P = sparsified_ppr(G, k, alpha=ALPHA, tol=TOL)
    assert P.shape == (n, n) and P.nnz == n * k
    ip = P.indptr.cpu().numpy()
    ix = P.indices.cpu().numpy()
    assert ip[0] == 0 and ip[-1] == n * k
    row = np.repeat(np.arange(n), np.diff(ip))
    same_row = row[1:] == row[:-1]
    assert (np.diff(ix.astype(np.int64))[same_row] > 0).all(), "CSR not canonical"
    assert np.array_equal(np.bincount(ix, minlength=n), np.full(n, k)), "not k per column"
    mask, vals = dense_mask(P)
    thresh = -np.partition(-Pi, k - 1, axis=1)[:, k - 1]  # k-th largest of every row
    # per column j against thresh[j]: work on the transposes so that a "row" is a column of Pi
    check_membership(mask.T, vals.T, Pi.T, thresh[:, None], E, k, np.full((n, 1), E),
                     "sparsified_ppr sym k=32")
    # the cached transpose is the CSC it was built from
    tp, tx, tv = P.transpose()
    assert np.array_equal(tp.cpu().numpy(), k * np.arange(n + 1))


@pytest.fixture(scope="module")
def quirk(graphs):
    """batch_topk_quirk (existing code) and its sparse form."""
    from ppnp_amd.ppr import SparsePPR, batch_topk_quirk

    P_dense = batch_topk_quirk(graphs["sym"], 32)
    return P_dense, SparsePPR.from_dense(P_dense)


def test_sparse_ppr_batch_matches_the_dense_protocol(cora, quirk):
    P_dense, S = quirk
    idx = torch.from_numpy(cora["split_a_train"][:64]).to(DEV)
    sub, sel = S.batch(idx)
    ppr_sub = P_dense[idx]                      # batch-main.py:140-142
    mask = (ppr_sub > 0).any(dim=0)
    assert torch.equal(sel, mask.nonzero().flatten())
    assert sub.shape == (64, int(mask.sum()))
    assert torch.equal(sub.to_dense(), ppr_sub[:, mask])
    assert torch.equal(S.rows(idx).to_dense(), ppr_sub)


@pytest.mark.parametrize("model_name", ["PPNP", "APPNP"])
def test_product_parity_with_the_dense_call(cora, adj, quirk, model_name):
    """model(X[sel], ppr=P_sub) and the encoder-weight gradients: SparsePPR against the dense
    ``ppr=P_dense[idx][:, sel]`` call, same weights, no dropout, the project's fp32 bound."""
    pa = _pa()
    P_dense, S = quirk
    n = int(cora["n"])
    idx = torch.from_numpy(cora["split_a_train"][:64]).to(DEV)
    sub, sel = S.batch(idx)
    gen = torch.Generator().manual_seed(9)
    X = torch.rand(n, 96, generator=gen).to(DEV)
    cot = torch.randn(64, 7, generator=gen).to(DEV)
    torch.manual_seed(3)
    if model_name == "PPNP":
        model = pa.PPNP(96, 7, ppr=torch.zeros(1, 1), drop_prob=0.0).to(DEV)
    else:
        model = pa.APPNP(96, 7, adj, drop_prob=0.0).to(DEV)
    model.train()
    params = [p for p in model.encoder.parameters()]

    def run(ppr):
        for p in params:
            p.grad = None
        out = model(X[sel], ppr=ppr)
        (out * cot).sum().backward()
        return out.detach(), [p.grad.detach().clone() for p in params]

    ref_out, ref_g = run(P_dense[idx][:, sel])
    out, g = run(sub)
    pairs = [("logits", out, ref_out)] + [(f"grad {i}", a, b) for i, (a, b) in
                                          enumerate(zip(g, ref_g))]
    for name, a, b in pairs:
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        print(f"{model_name} {name}: err {err:.3e}, bar {1e-5 * scale + 1e-6:.3e}")
        assert scale > 0
        assert err <= 1e-5 * scale + 1e-6, name


def test_trainer_runs_the_minibatch_protocol(monkeypatch):
    from ppnp_amd import train

    common = ["--dataset", "cora_ml", "--n-runs", "1", "--max-epochs", "3"]
    s = train.main(common + ["--batch-size", "32", "--ppr-topk", "32"])
    assert s["batch_size"] == 32 and s["ppr_topk"] == 32 and s["runs"] == 1
    assert len(s["records"]) == 1
    for rec in s["records"]:
        assert set(rec) == {"epoch", "elapsed", "stop_acc", "valid_acc"}  # batch-main.py:171-176
        assert all(np.isfinite(v) for v in rec.values())
        assert 0.0 <= rec["valid_acc"] <= 1.0
    assert np.isfinite(s["valid_acc_mean"]) and s["ppr_build_mean"] > 0

    # without --batch-size the full-batch path runs, and the minibatch loop is never entered
    def boom(*a, **kw):
        raise AssertionError("minibatch path taken")

    monkeypatch.setattr(train, "_run_batches", boom)
    s = train.main(common)
    assert "batch_size" not in s and np.isfinite(s["valid_acc_mean"])
