"""GPU: the top k straight from the forward push (ops.push_topk / appnp_push_topk), bit for bit.

Every case is compared with BOTH the numpy reference (tests/push_topk_ref.py: the replayed block,
the fp32 scales, a stable argsort of (-v, index)) and the device chain it replaces
(ops.push_columns -> ops.topk_columns) on the same inputs: the indices, the value bits, ``rounds``
and ``left``.  'sym' runs without scales, 'rw' with the row and column scales ppr.topk_rows
applies (degrees and inverse degrees).  The raw calls write into outputs with leading dimension
k + 3 whose padding holds a sentinel, and keep their workspace, so a later call finds whatever the
sources before it left in the slots.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import push_topk_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALPHA = 0.1
PAD = 3
IDX_SENTINEL, VAL_SENTINEL = -7, 777.0


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


def scales(G, sources):
    """(row_scale, col_scale) device tensors: None for 'sym'; for 'rw' what ppr.topk_rows passes,
    D and 1 / D[source] in fp32 (a source out of range takes node 0's: its row is all zero)."""
    if G.mode == "sym":
        return None, None
    dinv = G.csr()[3]
    src = torch.as_tensor(np.asarray(sources, dtype=np.int64), device=DEV)
    src = torch.where((src >= 0) & (src < G.n), src, torch.zeros_like(src))
    return (1.0 / dinv).float(), dinv[src].float()


def host(t):
    return None if t is None else t.cpu().numpy()


def reference(G, sources, eps, k, max_rounds=1000):
    """(idx, val, rounds, left, V) of the numpy reference, read-only."""
    ip, ix, v, w = walked(G)
    rs, cs = scales(G, sources)
    ref = push_topk_ref.push_topk(ip, ix, v, sources, ALPHA, eps, k, w, max_rounds, host(rs),
                                  host(cs))
    for a in ref:
        a.setflags(write=False)
    return ref


def chain(G, sources, eps, k, max_rounds=1000):
    """The device chain the entry point replaces, on the same arguments."""
    from ppnp_amd import ops

    idx = torch.as_tensor(np.asarray(sources, dtype=np.int64), device=DEV)
    rs, cs = scales(G, sources)
    X, rounds, left = ops.push_columns(G, idx, ALPHA, eps, max_rounds)
    i, v = ops.topk_columns(X, k, rs, cs)
    return host(i), host(v), host(rounds), host(left)


class Call:
    """One raw appnp_push_topk call's device buffers; ``launch`` may be repeated (the workspace is
    kept, and is poisoned once: the call has to clear what it relies on)."""

    def __init__(self, G, sources, eps, k, slots, max_rounds=1000):
        from ppnp_amd import _lib

        self.L, self.lib, self.G = _lib, _lib.load(), G
        self.src = torch.as_tensor(np.asarray(sources, dtype=np.int64), device=DEV)
        self.b, self.k, self.slots = int(self.src.numel()), int(k), int(slots)
        self.eps, self.max_rounds = eps, max_rounds
        self.rs, self.cs = scales(G, sources)
        self.ld = self.k + PAD
        self.idx = torch.empty((self.b, self.ld), dtype=torch.int32, device=DEV)
        self.val = torch.empty((self.b, self.ld), dtype=torch.float32, device=DEV)
        self.rounds = torch.empty(self.b, dtype=torch.int32, device=DEV)
        self.left = torch.empty(self.b, dtype=torch.int32, device=DEV)
        self.ws_bytes = int(self.lib.appnp_push_topk_workspace_bytes(G.n, self.slots))
        self.ws = torch.full((max(self.ws_bytes, 1),), 0xA5, dtype=torch.uint8, device=DEV)
        self.poison()

    def poison(self):
        self.idx.fill_(IDX_SENTINEL)
        self.val.fill_(VAL_SENTINEL)
        self.rounds.fill_(-5)
        self.left.fill_(-5)

    def launch(self, max_rounds=None):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        with torch.cuda.device(DEV):
            return self.lib.appnp_push_topk(
                self.G.handle, p(self.src), self.b, ALPHA, self.eps,
                self.max_rounds if max_rounds is None else max_rounds, self.k, p(self.rs),
                p(self.cs), p(self.idx), p(self.val), self.ld, p(self.rounds), p(self.left),
                self.slots, p(self.ws), self.ws_bytes,
                C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))

    def result(self):
        """(idx, val, rounds, left) after checking that the padding was not written."""
        torch.cuda.synchronize(DEV)
        idx, val = host(self.idx), host(self.val)
        assert (idx[:, self.k:] == IDX_SENTINEL).all(), "out_idx padding written"
        assert (val[:, self.k:] == VAL_SENTINEL).all(), "out_val padding written"
        return (np.ascontiguousarray(idx[:, :self.k]), np.ascontiguousarray(val[:, :self.k]),
                host(self.rounds), host(self.left))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, tag):
    """indices, value bits, rounds and left of two (idx, val, rounds, left, ...) results."""
    assert np.array_equal(got[2], want[2]), f"{tag}: rounds {got[2]} != {want[2]}"
    assert np.array_equal(got[3], want[3]), f"{tag}: left {got[3]} != {want[3]}"
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
    assert bad.size == 0, f"{tag}: indices differ in rows {bad[:8]} of {got[0].shape[0]}"
    bad = np.flatnonzero((bits(got[1]) != bits(want[1])).any(axis=1))
    assert bad.size == 0, f"{tag}: values differ in rows {bad[:8]} of {got[1].shape[0]}"


def check(G, sources, eps, k, slots, max_rounds=1000, ref=None):
    """One raw call against the reference and the device chain; returns (call, result)."""
    call = Call(G, sources, eps, k, slots, max_rounds)
    assert call.launch() == call.L.APPNP_OK
    got = call.result()
    same(got, reference(G, sources, eps, k, max_rounds) if ref is None else ref, "reference")
    same(got, chain(G, sources, eps, k, max_rounds), "device chain")
    assert (np.diff(got[0].astype(np.int64), axis=1) > 0).all(), "rows not strictly ascending"
    return call, got


# ---- Cora-ML ------------------------------------------------------------------------------------


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
    """The recipe of tests/test_gpu_push.py: 128 sources, the hub first, the minimum-degree node,
    a duplicated source and two indices out of range within the first 33."""
    n = adj.shape[0]
    deg = np.asarray(adj.sum(axis=1)).ravel()
    src = np.random.default_rng(23).choice(n, 128, replace=False).astype(np.int64)
    src[0] = int(deg.argmax())
    src[1] = int(deg.argmin())
    src[9] = src[4]
    src[12] = n + 3
    src[20] = -1
    src[31] = src[0]
    return src


@pytest.fixture(scope="module")
def cora_ref(graphs, cora_sources):
    """The reference of all 128 sources per (mode, eps, k), computed once and left unchanged; the
    smaller calls are its leading rows.  Every case must hold short rows and ties at the k-th
    value, or it no longer tests the padding and the tie rule."""
    cache = {}

    def get(mode, eps, k):
        if (mode, eps, k) not in cache:
            ref = reference(graphs[mode], cora_sources, eps, k)
            short, tied = push_topk_ref.short_and_tied(ref[4], k)
            print(f"{mode} eps {eps:g} k {k}: {int(short.sum())} short columns, "
                  f"{int(tied.sum())} tied at k")
            assert short.any() and tied.any(), (mode, eps, k, int(short.sum()), int(tied.sum()))
            cache[(mode, eps, k)] = ref
        return cache[(mode, eps, k)]

    return get


def lead(ref, b):
    return tuple(a[:b] for a in ref[:4])


def slot_count(slots, b):
    return b if slots == "b" else slots


@pytest.mark.parametrize("mode", ["sym", "rw"])
@pytest.mark.parametrize("eps,k", [(1e-3, 128), (1e-4, 32)])
@pytest.mark.parametrize("b", [1, 33, 128])
@pytest.mark.parametrize("slots", [1, 3, "b"])
def test_cora_matches_the_reference_and_the_chain(graphs, cora_sources, cora_ref, mode, eps, k, b,
                                                  slots):
    """slots < b: a source gives the same row whichever sources ran on its slot before it."""
    ref = lead(cora_ref(mode, eps, k), b)
    _, got = check(graphs[mode], cora_sources[:b], eps, k, slot_count(slots, b), ref=ref)
    assert got[2][0] > 0 and got[3][0] == 0
    if b >= 33:
        for c in (12, 20):  # out of range: the indices 0 .. k-1, zeros, left = -1
            assert got[3][c] == -1 and got[2][c] == 0
            assert np.array_equal(got[0][c], np.arange(k)) and not bits(got[1][c]).any()
        assert np.array_equal(got[0][9], got[0][4]) and np.array_equal(got[0][31], got[0][0])


@pytest.mark.parametrize("mode", ["sym", "rw"])
@pytest.mark.parametrize("slots", [1, 3, "b"])
def test_cora_small_eps(graphs, cora_sources, cora_ref, mode, slots):
    b = 33
    check(graphs[mode], cora_sources[:b], 1e-5, 128, slot_count(slots, b),
          ref=lead(cora_ref(mode, 1e-5, 128), b))


# ---- slot reuse and edge cases --------------------------------------------------------------


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_sources_cut_short_leave_their_slot_clean(graphs, cora_sources, mode):
    """max_rounds = 1: every source stops with a non-empty frontier and residuals all over its
    neighbourhood, and the next source on the slot is still exact; then the same call with
    max_rounds = 1000 on the same workspace."""
    G, k = graphs[mode], 16
    src = np.asarray(cora_sources[:8]).clip(0, G.n - 1)
    call, got = check(G, src, 1e-4, k, 2, max_rounds=1)
    assert (got[2] == 1).all() and (got[3] > 0).all()
    rs, cs = (host(t) for t in scales(G, src))
    a = np.float64(np.float32(ALPHA))
    x = np.float32(np.float64(int(2.0 ** 44 * a)) * 2.0 ** -44)
    for c, s in enumerate(src):  # alpha at the source, padded with zeros
        v = x if rs is None else (x * rs[s]) * cs[c]
        pad = [j for j in range(k) if j != s][:k - 1]
        assert np.array_equal(got[0][c], np.sort(np.r_[pad, s]).astype(np.int32))
        want = np.where(got[0][c] == s, v, np.float32(0)).astype(np.float32)
        assert np.array_equal(bits(got[1][c]), bits(want))
    call.poison()
    assert call.launch(max_rounds=1000) == call.L.APPNP_OK
    full = call.result()
    same(full, reference(G, src, 1e-4, k), "reference after the cut-short call")
    same(full, chain(G, src, 1e-4, k), "device chain after the cut-short call")
    assert (full[3] == 0).all()


@pytest.fixture(scope="module")
def star():
    n = 70_001
    leaves = np.arange(1, n)
    zero = np.zeros(n - 1, dtype=np.int64)
    return sp.csr_matrix((np.ones(2 * (n - 1), dtype=np.float32),
                          (np.r_[zero, leaves], np.r_[leaves, zero])), shape=(n, n))


@pytest.fixture(scope="module")
def star_graphs(star):
    return {m: _pa().Graph.from_scipy(star, mode=m, device=DEV, transpose=True)
            for m in ("sym", "rw")}


@pytest.fixture(scope="module")
def star_ref(star_graphs):
    """The reference of the star per (mode, k), computed once."""
    cache = {}

    def get(mode, k):
        if mode not in cache:  # one replay per mode; the selection per k is cheap
            cache[mode] = reference(star_graphs[mode], [0, 5, 0], 1e-4, 1)
        _, _, rounds, left, V = cache[mode]
        return push_topk_ref.select(V, k) + (rounds, left)

    return get


@pytest.mark.parametrize("mode", ["sym", "rw"])
@pytest.mark.parametrize("k", [1, 128, 1024])
def test_star_has_more_candidates_than_lds_holds(star_graphs, star_ref, mode, k):
    """70,001 taken nodes per source; all leaves tie, so the lowest indices win; the centre's row
    of 70,001 entries is walked in the clean-up before source 2 reuses slot 0."""
    _, got = check(star_graphs[mode], [0, 5, 0], 1e-4, k, 2, ref=star_ref(mode, k)[:4])
    assert (got[3] == 0).all()
    assert np.array_equal(got[0][0], got[0][2]) and np.array_equal(bits(got[1][0]), bits(got[1][2]))
    if k > 2:  # the leaves of the centre's row tie: a run of the lowest indices
        assert np.array_equal(got[0][0], np.arange(k))


def kat_graph(kat, name, mode):
    n = len(kat[f"{name}_indptr"]) - 1
    return _pa().Graph.from_csr(kat[f"{name}_indptr"], kat[f"{name}_indices"],
                                kat[f"{name}_data"], n, mode=mode, device=DEV, transpose=True)


@pytest.mark.parametrize("mode", ["sym", "rw"])
@pytest.mark.parametrize("name", ["weighted4", "complete5"])
@pytest.mark.parametrize("k", [1, "n"])
def test_kat_graphs_with_k_one_and_k_n(kat, name, mode, k):
    G = kat_graph(kat, name, mode)
    k = G.n if k == "n" else k
    for slots in (1, G.n):
        _, got = check(G, np.arange(G.n), 1e-4, k, slots)
        assert (got[3] == 0).all()
        if k == G.n:
            assert (got[0] == np.arange(G.n)).all()


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_isolated_node_gives_a_padded_row(kat, mode):
    """Node 2 of isolated3 has its self loop only: 88 rounds on one node, one positive entry."""
    G = kat_graph(kat, "isolated3", mode)
    _, got = check(G, [2, 0, 1], 1e-4, 2, 1)
    assert got[2][0] == 88 and (got[3] == 0).all()
    assert got[0][0].tolist() == [0, 2] and got[1][0][0] == 0 and got[1][0][1] > 0


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_increments_that_truncate_to_zero_record_a_node_once(kat, mode):
    """complete2 at eps = 1e-13: late in the run t < 1 / alpha and (int64)(t alpha) is 0, so
    "p was 0 before the add" would not identify a node's first take.  One slot, sources 0, 1, 0:
    columns 0 and 2 are equal and match the chain."""
    G = kat_graph(kat, "complete2", mode)
    for k in (1, 2):
        _, got = check(G, [0, 1, 0], 1e-13, k, 1)
        assert (got[3] == 0).all() and (got[2] > 100).all()
        assert np.array_equal(got[0][0], got[0][2])
        assert np.array_equal(bits(got[1][0]), bits(got[1][2]))


# ---- determinism and capture -----------------------------------------------------------------


def test_two_calls_give_the_same_bits(graphs, cora_sources):
    a = Call(graphs["sym"], cora_sources[:33], 1e-5, 128, 3)
    assert a.launch() == a.L.APPNP_OK
    first = a.result()
    a.poison()
    assert a.launch() == a.L.APPNP_OK
    same(a.result(), first, "second call on the same workspace")
    b = Call(graphs["sym"], cora_sources[:33], 1e-5, 128, 33)
    assert b.launch() == b.L.APPNP_OK
    same(b.result(), first, "another slot count")


def test_captured_call_replays_to_the_same_bits(graphs, cora_sources, cora_ref):
    G, b, eps, k = graphs["rw"], 33, 1e-3, 128
    ref = lead(cora_ref("rw", eps, k), b)
    call = Call(G, cora_sources[:b], eps, k, 3)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        assert call.launch() == call.L.APPNP_OK  # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call.launch() == call.L.APPNP_OK
    for _ in range(2):
        call.poison()
        call.ws.fill_(0x5A)
        g.replay()
        same(call.result(), ref, "replay")


# ---- refusals and limits -----------------------------------------------------------------------


def raw_refusal(G, k=2):
    """The raw call with valid buffers: (return code, outputs untouched)."""
    call = Call(G, [0, 1], 1e-4, k, 2, max_rounds=10)
    rc = call.launch()
    torch.cuda.synchronize(DEV)
    untouched = bool((call.idx == IDX_SENTINEL).all()) and bool((call.val == VAL_SENTINEL).all())
    return rc, untouched


def test_refusals(adj, kat):
    from ppnp_amd import _lib, ops

    pa = _pa()
    G = pa.Graph.from_scipy(adj, mode="rw", device=DEV)  # no transpose
    assert raw_refusal(G) == (_lib.APPNP_ENOTSUP, True)
    with pytest.raises(ValueError, match="transpose=True"):
        ops.push_topk(G, [0, 1], 4)
    # a directed graph: 0 -> 1, 1 -> 2, 2 -> 0
    d = sp.csr_matrix((np.ones(3, dtype=np.float32), ([0, 1, 2], [1, 2, 0])), shape=(3, 3))
    for mode in ("sym", "rw"):
        G = pa.Graph.from_scipy(d, mode=mode, device=DEV, transpose=True)
        assert not G.symmetric
        assert raw_refusal(G) == (_lib.APPNP_ENOTSUP, True)
        with pytest.raises(ValueError, match="undirected"):
            ops.push_topk(G, [0], 1)
    # a row partition of an undirected graph
    G = pa.Graph.from_scipy(adj, mode="sym", device=DEV, row_lo=0, row_hi=adj.shape[0] // 2)
    assert raw_refusal(G) == (_lib.APPNP_ENOTSUP, True)
    with pytest.raises(ValueError, match="row-partitioned"):
        ops.push_topk(G, [0], 1)
    # a valid graph passes the same raw call
    rc, untouched = raw_refusal(kat_graph(kat, "complete5", "rw"))
    assert rc == _lib.APPNP_OK and not untouched


def test_k_above_the_cap_is_refused_and_writes_nothing(graphs):
    from ppnp_amd import _lib, ops

    G = graphs["sym"]
    assert G.n > ops.PUSH_TOPK_MAX_K + 1
    assert raw_refusal(G, k=ops.PUSH_TOPK_MAX_K + 1) == (_lib.APPNP_ENOTSUP, True)
    with pytest.raises(ValueError, match="at most k = 1024"):
        ops.push_topk(G, [0, 1], ops.PUSH_TOPK_MAX_K + 1)
    # the cap itself is supported
    check(G, [0, G.n - 1], 1e-4, ops.PUSH_TOPK_MAX_K, 2)


# ---- end-to-end routes -------------------------------------------------------------------------


def same_sparse(P, Q):
    assert P.shape == Q.shape
    assert torch.equal(P.indptr, Q.indptr) and torch.equal(P.indices, Q.indices)
    assert torch.equal(P.data.view(torch.int32), Q.data.view(torch.int32))


@pytest.mark.parametrize("mode", ["sym", "rw"])
def test_topk_rows_lists_equal_block(graphs, mode):
    from ppnp_amd.ppr import topk_rows

    G, k, eps = graphs[mode], 32, 1e-4
    idx = torch.from_numpy(np.sort(np.random.default_rng(31).choice(G.n, 160, replace=False)))
    idx = idx.to(DEV)
    info_l, info_b = [], []
    P = topk_rows(G, idx, k, alpha=ALPHA, eps=eps, info=info_l, select="lists", chunk=7)
    Q = topk_rows(G, idx, k, alpha=ALPHA, eps=eps, info=info_b, select="block")
    same_sparse(P, Q)
    assert len(info_l) == 1 and len(info_b) == 2  # one call; chunks of 128 and 32
    assert tuple(info_l[0][0].shape) == (160,) and not bool(info_l[0][1].any())
    assert torch.equal(info_l[0][0], torch.cat([r for r, _ in info_b]))
    assert np.array_equal(P.indptr.cpu().numpy(), k * np.arange(161))


def test_sparsified_ppr_lists_equal_block(graphs, cora):
    from ppnp_amd.ppr import sparsified_ppr

    G, k, eps = graphs["sym"], 16, 1e-3
    info = []
    P = sparsified_ppr(G, k, alpha=ALPHA, eps=eps, select="lists", info=info)
    Q = sparsified_ppr(G, k, alpha=ALPHA, eps=eps, select="block")
    assert len(info) == 1 and info[0][0].numel() == G.n
    assert P.shape == (G.n, G.n) and P.nnz == G.n * k
    idx = torch.from_numpy(cora["split_a_train"][:64]).to(DEV)
    (sub, sel), (rsub, rsel) = P.batch(idx), Q.batch(idx)
    assert torch.equal(sel, rsel)
    same_sparse(sub, rsub)
    same_sparse(P, Q)


def test_one_push_launch_covers_160_sources(graphs):
    from ppnp_amd import ops

    idx = torch.arange(160, device=DEV)
    for mode, want in (("sym", ["copy", "copy", "push"]), ("rw", ["copy", "push"])):
        times = ops.kernel_times(lambda: ops.push_topk(graphs[mode], idx, 32), DEV)
        assert [kind for kind, _ in times] == want
        assert all(ms >= 0 for _, ms in times)


def test_default_slots_follow_the_sources_and_the_device(graphs):
    from ppnp_amd import ops

    G = graphs["sym"]
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert ops.push_topk_slots(G, 5) == 5
    assert ops.push_topk_slots(G, 10 * cus) == cus
    i, v, rounds, left = ops.push_topk(G, torch.arange(5, device=DEV), 8)
    want = chain(G, np.arange(5), 1e-4, 8)
    same((host(i), host(v), host(rounds), host(left)), want, "ops.push_topk against the chain")


def test_trainer_runs_an_epoch_on_list_selected_rows(monkeypatch):
    from ppnp_amd import train

    losses = []
    cross_entropy = train.F.cross_entropy

    def recording(*a, **kw):
        losses.append(cross_entropy(*a, **kw))
        return losses[-1]

    monkeypatch.setattr(train.F, "cross_entropy", recording)
    s = train.main(["--dataset", "cora_ml", "--n-runs", "1", "--max-epochs", "1",
                    "--batch-size", "32", "--ppr-topk", "32", "--ppr-eps", "1e-4",
                    "--ppr-select", "lists"])
    assert s["ppr_eps"] == 1e-4 and s["ppr_select"] == "lists" and s["runs"] == 1
    rec = s["records"][0]
    assert len(losses) >= 2  # the training batches and the stopping set
    assert all(np.isfinite(float(v.detach())) for v in losses)
    assert all(np.isfinite(v) for v in rec.values())
    assert 0.0 <= rec["valid_acc"] <= 1.0 and s["ppr_build_mean"] > 0
