"""GPU: PPR columns by forward push (ops.push_columns / appnp_push_columns) against the numpy
replay of the same fixed-point algorithm (tests/push_ref.py).

Every sum of the algorithm is an integer sum and a round is a pure function of the state before
it, so the comparison is exact: the bit patterns of X, and ``rounds`` and ``left`` as integers.
The replay walks what the kernel walks: the CSR the graph holds (its fp32 values and fp64 inverse
degrees are read back with ``Graph.csr``), transposed on the host for 'rw'.  X is written into
the first b columns of a block with leading dimension b + 5 whose padding holds a sentinel.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import push_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALPHA = 0.1
PAD = 5
SENTINEL = -7.25


def _pa():
    import ppnp_amd

    return ppnp_amd


def walked(G):
    """(indptr, indices, fp32 vals of A_hat^T, threshold weights w or None) as the kernel
    reads them."""
    rp, col, val, dinv = (t.cpu().numpy() for t in G.csr())
    if G.mode == "sym":
        return rp, col, val, 1.0 / dinv
    at = sp.csr_matrix((val, col, rp), shape=(G.n, G.n)).T.tocsr()
    return at.indptr, at.indices, at.data, None


def replay(G, sources, eps, max_rounds=1000):
    ip, ix, v, w = walked(G)
    return push_ref.push_columns(ip, ix, v, sources, ALPHA, eps, w, max_rounds)


def run(G, sources, eps, max_rounds=1000):
    """push_columns into a padded block; (X, rounds, left) as numpy, the padding checked."""
    from ppnp_amd import ops

    idx = torch.as_tensor(np.asarray(sources, dtype=np.int64), device=DEV)
    b = int(idx.numel())
    buf = torch.full((G.n, b + PAD), SENTINEL, dtype=torch.float32, device=DEV)
    X, rounds, left = ops.push_columns(G, idx, ALPHA, eps, max_rounds, out=buf[:, :b])
    assert X.data_ptr() == buf.data_ptr()
    assert bool((buf[:, b:] == SENTINEL).all()), "padding columns written"
    return X.cpu().numpy(), rounds.cpu().numpy(), left.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


def check(G, sources, eps, max_rounds=1000, ref=None):
    X, rounds, left = run(G, sources, eps, max_rounds)
    Xr, rr, lr, _ = replay(G, sources, eps, max_rounds) if ref is None else ref
    assert np.array_equal(rounds, rr), (rounds, rr)
    assert np.array_equal(left, lr), (left, lr)
    assert same_bits(X, Xr), f"{int((X.view(np.uint32) != Xr.view(np.uint32)).sum())} differ"
    return X, rounds, left


@pytest.fixture(scope="module")
def adj(cora):
    n = int(cora["n"])
    return sp.csr_matrix((cora["adj_data"], cora["adj_indices"], cora["adj_indptr"]), shape=(n, n))


@pytest.fixture(scope="module")
def graphs(adj):
    pa = _pa()
    return {m: pa.Graph.from_scipy(adj, mode=m, device=DEV, transpose=True)
            for m in ("sym", "rw")}


@pytest.fixture(scope="module")
def cora_sources(adj):
    """128 sources: the hub first, a duplicated source and two indices out of range within the
    first 33."""
    n = adj.shape[0]
    deg = np.asarray(adj.sum(axis=1)).ravel()
    src = np.random.default_rng(23).choice(n, 128, replace=False).astype(np.int64)
    src[0] = int(deg.argmax())
    src[1] = int(deg.argmin())
    src[9] = src[4]      # a duplicate: an independent column
    src[12] = n + 3      # out of range
    src[20] = -1
    src[31] = src[0]     # the hub again
    return src


@pytest.fixture(scope="module")
def cora_ref(graphs, cora_sources):
    """The replay of all 128 sources per (mode, eps), computed once and left unchanged; the
    smaller blocks are its leading columns."""
    cache = {}

    def get(mode, eps):
        if (mode, eps) not in cache:
            ref = replay(graphs[mode], cora_sources, eps)
            for a in ref:
                a.setflags(write=False)
            cache[(mode, eps)] = ref
        return cache[(mode, eps)]

    return get


@pytest.mark.parametrize("mode", ["sym", "rw"])
@pytest.mark.parametrize("eps", [1e-3, 1e-5])
@pytest.mark.parametrize("b", [1, 33, 128])
def test_cora_matches_the_replay(graphs, cora_sources, cora_ref, mode, eps, b):
    ref = tuple(a[..., :b] for a in cora_ref(mode, eps))
    X, rounds, left = check(graphs[mode], cora_sources[:b], eps, ref=ref)
    print(f"{mode} eps {eps:g} b {b}: rounds max {rounds.max()}, edges {int(ref[3].sum())}")
    assert rounds[0] > 0 and left[0] == 0
    if b >= 33:
        assert left[12] == -1 and left[20] == -1 and rounds[12] == 0
        assert not X[:, 12].any() and not X[:, 20].any()
        assert same_bits(X[:, 9], X[:, 4]) and same_bits(X[:, 31], X[:, 0])
        ok = np.ones(b, dtype=bool)
        ok[[12, 20]] = False
        assert (left[ok] == 0).all()


def kat_graph(kat, name, mode):
    n = len(kat[f"{name}_indptr"]) - 1
    return _pa().Graph.from_csr(kat[f"{name}_indptr"], kat[f"{name}_indices"],
                                kat[f"{name}_data"], n, mode=mode, device=DEV, transpose=True)


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_isolated_node_pushes_into_its_own_zeroed_slot(kat, mode):
    """Node 2 of isolated3 has its self loop only (A_hat[2, 2] = 1): each round takes r_2 and
    adds 0.9 r_2 back into the slot zeroed in the same round, until 0.9^k < 1e-4: k = 88."""
    G = kat_graph(kat, "isolated3", mode)
    X, rounds, left = check(G, [2, 0, 1], 1e-4)
    assert rounds[0] == 88 and (left == 0).all()
    assert X[0, 0] == 0 and X[1, 0] == 0
    ref = kat[f"isolated3_ppr_{mode}_a0.1"][:, [2, 0, 1]]
    assert (np.abs(ref - X.astype(np.float64)) < 1e-4 * np.sqrt(2.0)).all()


@pytest.mark.parametrize("mode", ["sym", "rw"])
@pytest.mark.parametrize("name", ["weighted4", "complete5"])
def test_kat_graphs_match_the_replay_and_the_bound(kat, name, mode):
    G = kat_graph(kat, name, mode)
    n = G.n
    eps = 1e-4
    X, rounds, left = check(G, np.arange(n), eps)
    assert (left == 0).all() and (rounds > 0).all()
    w = walked(G)[3]
    w = np.ones(n) if w is None else w
    err = np.abs(kat[f"{name}_ppr_{mode}_a0.1"] - X.astype(np.float64)) / w[:, None]
    print(f"{name} {mode}: rounds {rounds}, max |err| / (eps w) {err.max() / eps:.3f}")
    assert err.max() < eps


@pytest.fixture(scope="module")
def star():
    n = 70_001
    leaves = np.arange(1, n)
    zero = np.zeros(n - 1, dtype=np.int64)
    return sp.csr_matrix((np.ones(2 * (n - 1), dtype=np.float32),
                          (np.r_[zero, leaves], np.r_[leaves, zero])), shape=(n, n))


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_star_hub_row_and_a_frontier_larger_than_the_workgroup(star, mode):
    """The centre's row has 70,001 entries (one wave walks it in chunks, or all waves together
    while the frontier is short), and the round after it has all 70,000 leaves in the frontier."""
    G = _pa().Graph.from_scipy(star, mode=mode, device=DEV, transpose=True)
    X, rounds, left = check(G, [0, 5, 0], 1e-4)
    assert (left == 0).all() and rounds[0] >= 2
    assert same_bits(X[:, 0], X[:, 2])
    assert X[1:, 0].min() > 0  # the centre's mass reached every leaf


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_one_round_leaves_alpha_at_the_source(graphs, cora_sources, mode):
    src = cora_sources[:4]
    X, rounds, left = check(graphs[mode], src, 1e-4, max_rounds=1)
    a = np.float64(np.float32(ALPHA))
    want = np.float32(np.float64(int(2.0 ** 44 * a)) * 2.0 ** -44)
    for c, s in enumerate(src):
        col = np.zeros(graphs[mode].n, dtype=np.float32)
        col[s] = want
        assert same_bits(X[:, c], col)
    assert (rounds == 1).all() and (left > 0).all()


def test_two_calls_give_the_same_bits(graphs, cora_sources):
    a = run(graphs["sym"], cora_sources[:33], 1e-5)
    b = run(graphs["sym"], cora_sources[:33], 1e-5)
    assert same_bits(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_captured_call_replays_to_the_same_bits(graphs, cora_sources, cora_ref):
    from ppnp_amd import ops

    G, b = graphs["rw"], 33
    ref = tuple(a[..., :b] for a in cora_ref("rw", 1e-3))
    idx = torch.as_tensor(cora_sources[:b], device=DEV)
    buf = torch.full((G.n, b + PAD), SENTINEL, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ops.push_columns(G, idx, ALPHA, 1e-3, out=buf[:, :b])  # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        X, rounds, left = ops.push_columns(G, idx, ALPHA, 1e-3, out=buf[:, :b])
    for _ in range(2):
        buf[:, :b] = float("nan")
        rounds.fill_(-5)
        left.fill_(-5)
        g.replay()
        torch.cuda.synchronize(DEV)
        assert same_bits(X.cpu().numpy(), ref[0])
        assert np.array_equal(rounds.cpu().numpy(), ref[1])
        assert np.array_equal(left.cpu().numpy(), ref[2])
        assert bool((buf[:, b:] == SENTINEL).all())


def raw_call(G, b=2):
    """appnp_push_columns itself, with valid buffers: its return code."""
    from ppnp_amd import _lib

    lib = _lib.load()
    idx = torch.zeros(b, dtype=torch.int64, device=DEV)
    X = torch.zeros(G.n, b, dtype=torch.float32, device=DEV)
    nb = int(lib.appnp_push_workspace_bytes(G.n, b))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.appnp_push_columns(G.handle, C.c_void_p(idx.data_ptr()), b, ALPHA, 1e-4, 10,
                                    C.c_void_p(X.data_ptr()), b, None, None,
                                    C.c_void_p(ws.data_ptr()), nb,
                                    C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize(DEV)
    return rc, X


def test_refusals(adj, kat):
    from ppnp_amd import _lib, ops

    pa = _pa()
    G = pa.Graph.from_scipy(adj, mode="rw", device=DEV)  # no transpose
    rc, X = raw_call(G)
    assert rc == _lib.APPNP_ENOTSUP and not X.any()
    with pytest.raises(ValueError, match="transpose=True"):
        ops.push_columns(G, [0, 1])
    # a directed graph: 0 -> 1, 1 -> 2, 2 -> 0
    d = sp.csr_matrix((np.ones(3, dtype=np.float32), ([0, 1, 2], [1, 2, 0])), shape=(3, 3))
    for mode in ("sym", "rw"):
        G = pa.Graph.from_scipy(d, mode=mode, device=DEV, transpose=True)
        assert not G.symmetric
        assert raw_call(G)[0] == _lib.APPNP_ENOTSUP
        with pytest.raises(ValueError, match="undirected"):
            ops.push_columns(G, [0])
    # a valid graph passes the same raw call
    assert raw_call(kat_graph(kat, "complete5", "rw"))[0] == _lib.APPNP_OK


def test_kernel_timer_names_the_push_launch(graphs, cora_sources):
    from ppnp_amd import ops

    idx = torch.as_tensor(cora_sources[:8].clip(0, graphs["sym"].n - 1), device=DEV)
    for mode, want in (("sym", ["copy", "copy", "push", "copy"]), ("rw", ["copy", "push", "copy"])):
        times = ops.kernel_times(lambda: ops.push_columns(graphs[mode], idx), DEV)
        assert [k for k, _ in times] == want
        assert all(ms >= 0 for _, ms in times)


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_topk_rows_equal_the_selection_of_the_replayed_block(graphs, mode):
    """topk_rows(eps=) = topk_columns of the replay's columns, chunk by chunk: indices and value
    bits (rw: through the same row and column scales)."""
    from ppnp_amd.ops import topk_columns
    from ppnp_amd.ppr import topk_rows

    G, k, eps = graphs[mode], 32, 1e-4
    idx = np.sort(np.random.default_rng(31).choice(G.n, 160, replace=False))
    info = []
    P = topk_rows(G, torch.from_numpy(idx).to(DEV), k, alpha=ALPHA, eps=eps, info=info)
    assert P.shape == (160, G.n) and len(info) == 2  # chunks of 128 and 32
    assert all(not bool(left.any()) for _, left in info)
    Xr = torch.from_numpy(replay(G, idx, eps)[0]).to(DEV)
    rs = cs = None
    if mode == "rw":
        dinv = G.csr()[3]
        rs, cs = (1.0 / dinv).float(), dinv[torch.from_numpy(idx).to(DEV)].float()
    ix, dv = [], []
    for s in (0, 128):
        i, v = topk_columns(Xr[:, s:s + 128].contiguous(), k, rs,
                            None if cs is None else cs[s:s + 128])
        ix.append(i.reshape(-1))
        dv.append(v.reshape(-1))
    assert torch.equal(P.indices, torch.cat(ix))
    assert torch.equal(P.data.view(torch.int32), torch.cat(dv).view(torch.int32))
    assert np.array_equal(P.indptr.cpu().numpy(), k * np.arange(161))


def test_sparsified_ppr_batch_equals_the_replay_built_matrix(graphs, cora):
    from ppnp_amd.ops import topk_columns
    from ppnp_amd.ppr import SparsePPR, sparsified_ppr

    G, k, eps = graphs["sym"], 16, 1e-3
    n = G.n
    P = sparsified_ppr(G, k, alpha=ALPHA, eps=eps)
    assert P.shape == (n, n) and P.nnz == n * k
    assert np.array_equal(np.bincount(P.indices.cpu().numpy(), minlength=n), np.full(n, k))
    # the same matrix from the replay's columns: top k of every column (a CSC), transposed
    Xr = torch.from_numpy(replay(G, np.arange(n), eps)[0]).to(DEV)
    i, v = topk_columns(Xr, k)
    indptr = torch.arange(n + 1, dtype=torch.int64, device=DEV) * k
    csc = SparsePPR(indptr, i.reshape(-1), v.reshape(-1), (n, n), device=DEV)
    R = SparsePPR(*csc.transpose(), (n, n), device=DEV)
    idx = torch.from_numpy(cora["split_a_train"][:64]).to(DEV)
    (sub, sel), (rsub, rsel) = P.batch(idx), R.batch(idx)
    assert torch.equal(sel, rsel) and sub.shape == rsub.shape
    assert torch.equal(sub.indptr, rsub.indptr) and torch.equal(sub.indices, rsub.indices)
    assert torch.equal(sub.data.view(torch.int32), rsub.data.view(torch.int32))


def test_trainer_runs_an_epoch_on_pushed_rows(monkeypatch):
    from ppnp_amd import train

    losses = []
    cross_entropy = train.F.cross_entropy

    def recording(*a, **kw):
        losses.append(cross_entropy(*a, **kw))
        return losses[-1]

    monkeypatch.setattr(train.F, "cross_entropy", recording)
    s = train.main(["--dataset", "cora_ml", "--n-runs", "1", "--max-epochs", "1",
                    "--batch-size", "32", "--ppr-topk", "32", "--ppr-eps", "1e-4"])
    assert s["ppr_eps"] == 1e-4 and s["runs"] == 1
    rec = s["records"][0]
    assert len(losses) >= 2  # the training batches and the stopping set
    assert all(np.isfinite(float(v.detach())) for v in losses)
    assert all(np.isfinite(v) for v in rec.values())
    assert 0.0 <= rec["valid_acc"] <= 1.0 and s["ppr_build_mean"] > 0
