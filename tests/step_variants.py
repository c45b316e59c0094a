"""Which instantiation of the fused step kernel a call reaches, and a table of cases that reaches
every vector-tail cell of it.  A plain module shared by tests/test_step_variants.py (CPU: the
table covers the cells), tests/test_gpu_vector_tails.py and tests/test_gpu_bf16_exact.py.

The vector-tail code of ppnp_amd/csrc/appnp_spmm.hip (the TAIL switches of frag_load /
frag_store, the piecewise read of a buffer's last row) runs only when F is not a multiple of V,
every leading dimension is a multiple of V, and launch_step keeps that V.  ``expected_variant``
mirrors those decisions on the host; ``CASES`` names, per cell (dtype, V, F mod V), a graph, a
width and a layout that lands in it.  profiles/step_variants_hit.txt records the instantiations
a kernel trace of the GPU modules saw, checked once against ``expected_kernel`` over CASES.
"""

import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from oracle import ppnp_oracle as O

# ---------------------------------------------------------------------------------------
# the dispatch, mirrored
# ---------------------------------------------------------------------------------------

K_WAVE = 64          # appnp_device.h kWave
K_HEAVY_ROW = 32     # kHeavyRow: a longer row gets a wavefront inside the narrow launch
K_HUB_ROW = 512      # kHubRow: a longer row is dispatched first by the wide launch
K_WIDE_AVG_ROW = 24  # kWideAvgRow
K_LATENCY_ROWS = 1 << 16


def line_ld(f, dtype):
    """appnp_internal.h line_ld / avg_lines: leading dimension of the internal buffers."""
    es = 4 if dtype == "fp32" else 2
    line = 128 // es

    def avg_lines(row_bytes, stride):
        g = 128 if stride % 128 == 0 else stride
        period = 128 // np.gcd(128, g)
        return sum(((i * stride) % 128 + row_bytes - 1) // 128 + 1 for i in range(period)) / period

    if f <= line:
        padded = 1
        while padded < f:
            padded <<= 1
    else:
        padded = (f + line - 1) // line * line
    v = 4 if es == 4 else 8
    packed = (f + v - 1) // v * v
    return padded if avg_lines(f * es, padded * es) < avg_lines(f * es, packed * es) else packed


def pick_vec(dtype, f, lds):
    """appnp_spmm.hip pick_vec, for base pointers that allow 16-B vectors (torch allocations and
    row views of them)."""
    v = 4 if dtype == "fp32" else 8
    while v > 1:
        if (v <= f or f % v == 0) and all(ld % v == 0 for ld in lds):
            break
        v >>= 1
    return v


def expected_variant(dtype, f, lds, n_rows, nnz, n_heavy, n_hub):
    """(V, G, wide, tail_rem, regime) of the launch, mirroring appnp_spmm.hip: pick_vec, then in
    launch_step the regime (``latency``), the shrinking of V (``if (latency && !heavy_rows)``),
    ``lanes_for``, ``long_rows`` and ``wide``.  ``n_heavy`` / ``n_hub`` are the row lists the
    call passes (0 for a step over part of the rows' entries: drop_row_lists); with n_heavy > 0
    a narrow launch appends wavefront-per-row blocks (``if (!wide && a.heavy ...)``), a wide one
    dispatches its n_hub rows first."""
    V = pick_vec(dtype, f, lds)
    latency = n_rows <= K_LATENCY_ROWS
    heavy_rows = n_heavy > 0
    if latency and not heavy_rows:
        v = 1
        while v < V and 64 * v < f:
            v <<= 1
        V = v
    need = (min(f, 64 * V) + V - 1) // V
    G = 1
    while G < need:
        G <<= 1
    long_rows = nnz >= K_WIDE_AVG_ROW * n_rows
    wide = G >= 16 or (latency and heavy_rows) or (not latency and long_rows)
    return V, G, wide, f % V, "latency" if latency else "bandwidth"


def runs_wave_row(variant, n_heavy):
    """The launch runs wave_row: a wide launch, or the heavy blocks of a narrow one."""
    return variant[2] or n_heavy > 0


EPI = {"FWD": 0, "BWD": 1, "PARTIAL": 2, "FINISH": 3, "ACCUM": 4, "CHEB": 5}


def expected_kernel(dtype, epi, variant, nnz, nnz_rows, n_rows, n_heavy):
    """The instantiation's name as a kernel trace prints it, k_step_wide / k_step_narrow
    <T, V, G, EPI, U, TAIL>: U mirrors ``uw`` / ``un`` of launch_step and launch_g."""
    V, G, wide, rem, regime = variant
    latency = regime == "latency"
    long_rows = nnz >= K_WIDE_AVG_ROW * n_rows
    long_whole = (nnz_rows or nnz) >= K_WIDE_AVG_ROW * n_rows
    if wide:
        U = 8 if (latency and n_heavy > 0) else 2 if (not latency and (long_rows or long_whole)) else 1
    else:
        U = 8 if (latency and V <= 2) else 4
    T = "float" if dtype == "fp32" else "unsigned short"
    return (f"k_step_{'wide' if wide else 'narrow'}<{T}, {V}, {G}, {EPI[epi]}, {U}, "
            f"{'true' if rem else 'false'}>")


# ---------------------------------------------------------------------------------------
# graphs (seeded; the shapes are asserted in tests/test_step_variants.py)
# ---------------------------------------------------------------------------------------

N_BIG = 66_000
ROWS_N, ROWS_LO, ROWS_HI = 2000, 300, 1500   # the row-range graph R holds rows [300, 1500)
ROWS_SHARDS, ROWS_SHARD_ROWS = 3, 700        # its source shards: columns [0, 700), .. [1400, 2000)


def _with_edges(adj, src, dst):
    n = adj.shape[0]
    extra = sp.coo_matrix((np.ones(len(src), np.float32), (src, dst)), shape=(n, n)).tocsr()
    a = ((adj + extra + extra.T) > 0).astype(np.float32).tocsr()
    a.setdiag(0)
    a.eliminate_zeros()
    a.sort_indices()
    return a


@functools.lru_cache(maxsize=None)
def adjacency(name):
    """L1: latency regime with heavy and hub rows.  Bs / Bsh / Bl: bandwidth regime with short
    rows, short rows plus heavy and hub rows, long rows.  R: the graph whose rows [300, 1500) a
    row-partitioned rank holds; its last held row reaches the last row of Zin and a row below
    the range.  Md: MS-Academic-sized.  D: directed (upper triangle)."""
    if name == "L1":
        from test_gpu_parity import _hub_graph

        return _hub_graph(n=4000)
    if name == "Bs":
        return O.synth_graph(N_BIG, 4 * N_BIG, 21)
    if name == "Bsh":
        rng = np.random.default_rng(31)
        rows = [7, 4099, 30_000, 47_111, N_BIG - 1, 12_345]
        counts = [40, 45, 50, 55, 60, 600]
        src = np.repeat(rows, counts)
        dst = np.concatenate([rng.choice(N_BIG, c, replace=False) for c in counts])
        return _with_edges(adjacency("Bs"), src, dst)
    if name == "Bl":
        return O.synth_graph(N_BIG, 14 * N_BIG, 22)
    if name == "R":
        return _with_edges(O.synth_graph(ROWS_N, 9000, 23), [ROWS_HI - 1, ROWS_HI - 1],
                           [ROWS_N - 1, 5])
    if name == "Md":
        return O.synth_graph(18333, 81894, 3)
    if name == "D":
        a = sp.triu(O.synth_graph(1200, 5000, 3), format="csr").astype(np.float32)
        a.sort_indices()
        return a
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def a_hat(name, mode="sym"):
    return O.calc_a_hat(adjacency(name), mode)


Stats = namedtuple("Stats", "n rows nnz n_heavy n_hub")


@functools.lru_cache(maxsize=None)
def stats(name, part="ALL"):
    """Host-only statistics of the entries a step multiplies: the held rows of the oracle's
    A_hat; LOCAL / REMOTE halves and shard ranges carry no heavy / hub lists."""
    ah = a_hat(name)
    n = ah.shape[0]
    if name != "R":
        lens = np.diff(ah.indptr)
        return Stats(n, n, int(ah.nnz), int((lens > K_HEAVY_ROW).sum()),
                     int((lens > K_HUB_ROW).sum()))
    rows = ROWS_HI - ROWS_LO
    held = ah[ROWS_LO:ROWS_HI]
    if part == "ALL":
        lens = np.diff(held.indptr)
        return Stats(n, rows, int(held.nnz), int((lens > K_HEAVY_ROW).sum()),
                     int((lens > K_HUB_ROW).sum()))
    if part == "LOCAL":
        return Stats(n, rows, int(held[:, ROWS_LO:ROWS_HI].nnz), 0, 0)
    if part == "REMOTE":
        return Stats(n, rows, int(held.nnz - held[:, ROWS_LO:ROWS_HI].nnz), 0, 0)
    s_lo, s_hi = part  # a shard range: its uniform share of the entries (shards_of)
    return Stats(n, rows, int(held.nnz) * (s_hi - s_lo) // ROWS_SHARDS, 0, 0)


# ---------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------

Case = namedtuple("Case", "graph dtype f ld epi p_drop ld_p")


def _cases():
    fwd = [
        # narrow rows (G <= 8) on Bs / Bsh; on Bsh the heavy rows run wave_row in the same launch
        ("Bs", "fp32", 13, 16), ("Bsh", "fp32", 14, 16), ("Bs", "fp32", 15, 16),
        ("Bsh", "fp32", 7, 10),
        ("Bs", "bf16", 9, 16), ("Bsh", "bf16", 10, 16), ("Bs", "bf16", 11, 16),
        ("Bsh", "bf16", 12, 16), ("Bs", "bf16", 13, 16), ("Bsh", "bf16", 14, 16),
        ("Bs", "bf16", 15, 16),
        ("Bsh", "bf16", 13, 20), ("Bs", "bf16", 14, 20), ("Bsh", "bf16", 15, 20),
        ("Bs", "bf16", 7, 10),
        # wide: G >= 16, the latency regime with heavy rows (L1), long rows (Bl)
        ("L1", "fp32", 101, 104), ("Bl", "fp32", 14, 16), ("Bs", "fp32", 67, 68),
        ("L1", "fp32", 7, 10), ("L1", "fp32", 131, 134),
        ("Bs", "bf16", 65, 72), ("L1", "bf16", 10, 16), ("Bl", "bf16", 11, 16),
        ("L1", "bf16", 100, 104), ("Bs", "bf16", 69, 72), ("Bl", "bf16", 70, 72),
        ("L1", "bf16", 15, 16), ("L1", "bf16", 13, 16),
        ("L1", "bf16", 13, 20), ("Bs", "bf16", 66, 68), ("Bl", "bf16", 7, 12),
        ("L1", "bf16", 7, 10),
    ]
    bwd = [
        ("L1", "fp32", 7, 10), ("Bsh", "fp32", 13, 16), ("L1", "fp32", 98, 104),
        ("Bl", "fp32", 15, 16),
        ("Bsh", "bf16", 7, 10), ("L1", "bf16", 13, 20), ("Bs", "bf16", 66, 68),
        ("Bl", "bf16", 7, 12),
        ("L1", "bf16", 9, 16), ("Bsh", "bf16", 10, 16), ("Bs", "bf16", 67, 72),
        ("L1", "bf16", 100, 104), ("Bl", "bf16", 13, 16), ("Bsh", "bf16", 14, 16),
        ("L1", "bf16", 71, 72),
    ]
    out = []
    for i, (g, dt, f, ld) in enumerate(fwd):
        out.append(Case(g, dt, f, ld, "FWD", 0.3 if i % 3 == 1 else 0.0, None))
    for i, (g, dt, f, ld) in enumerate(bwd):
        out.append(Case(g, dt, f, ld, "BWD", 0.3 if i % 3 == 1 else 0.0, None))
    # the fp32 partial chain of a row-partitioned step: 64 * 2 < F keeps V = 4 in the latency
    # regime; the partial has its own leading dimension
    for i, f in enumerate((129, 130, 131)):
        for j, epi in enumerate(("PARTIAL", "FINISH", "ACCUM")):
            out.append(Case("R", "fp32", f, 132, epi, 0.3 if (i + j) % 3 == 1 else 0.0, 136))
    return out


CASES = _cases()


def case_id(c):
    return f"{c.graph}-{c.dtype}-F{c.f}-ld{c.ld}-{c.epi}" + ("-drop" if c.p_drop else "")


def case_launches(c):
    """[(epi, lds, Stats)] of the step launches a case checks."""
    if c.epi == "FWD":
        return [("FWD", (c.ld, c.ld, c.ld), stats(c.graph))]
    if c.epi == "BWD":  # appnp_propagate_bwd counts the internal buffer's leading dimension
        return [("BWD", (c.ld, c.ld, line_ld(c.f, c.dtype)), stats(c.graph))]
    if c.epi == "PARTIAL":  # appnp_step PART_LOCAL; appnp_step_shards FIRST on the last shard
        return [("PARTIAL", (c.ld, c.ld_p), stats("R", "LOCAL")),
                ("PARTIAL", (c.ld, c.ld_p), stats("R", (2, 3)))]
    if c.epi == "FINISH":   # appnp_step PART_REMOTE
        return [("FINISH", (c.ld, c.ld, c.ld, c.ld_p), stats("R", "REMOTE"))]
    if c.epi == "ACCUM":    # appnp_step_shards ACC on shards [1, 3)
        return [("ACCUM", (c.ld, c.ld_p), stats("R", (1, 3)))]
    raise KeyError(c.epi)


def case_variants(c):
    return [(epi, expected_variant(c.dtype, c.f, lds, st.rows, st.nnz, st.n_heavy, st.n_hub), st)
            for epi, lds, st in case_launches(c)]


# one propagate_forward(K = 3) on padded views per (dtype, V): the internal line_ld buffer is the
# gather source of the middle iteration
FORWARD_K3 = [("L1", "fp32", 7, 10), ("L1", "fp32", 101, 104), ("L1", "bf16", 7, 10),
              ("Bsh", "bf16", 13, 20), ("L1", "bf16", 100, 104)]


# ---------------------------------------------------------------------------------------
# host references of the bf16 chains (numpy; used by the GPU modules)
# ---------------------------------------------------------------------------------------


def scaled_bf16(dZ, alpha):
    """dH_0 of the adjoint in bf16 storage, bit-exact: RNE(fl32(dZ * float32(alpha)))."""
    return O.round_bf16(np.asarray(dZ, dtype=np.float32) * np.float32(alpha))


def forward_chain_bf16(csr, H, K, alpha, p_drop=0.0, seed=0):
    """The bf16-emulating forward chain Z_k = RNE(step_exact(Z_{k-1})) and the envelope of any
    faithful implementation around it after K steps."""
    Z = np.asarray(H, dtype=np.float32)
    E = np.zeros(Z.shape)
    for k in range(K):
        t, delta = O.step_exact(*csr, Z, H, alpha, k, p_drop, seed)
        E = O.envelope(*csr, E, None, t, delta, alpha, k, p_drop, seed)
        Z = O.round_bf16(t.astype(np.float32))
    return Z, E


def backward_step_bf16(csr_t, G, dH, alpha, k, p_drop, seed):
    """(t, delta) of the adjoint's dH update at iteration k on A_hat^T (``csr_t``): dH <-
    a_k y + dH with y = s M_k^T G, a_k = alpha for k >= 1 and 1 for k = 0."""
    return O.step_exact(*csr_t, G, dH, alpha, k, p_drop, seed, transposed=True, h_weight=1.0,
                        y_weight=alpha if k >= 1 else None)


def backward_chain_bf16(csr_t, dZ, K, alpha, p_drop=0.0, seed=0):
    """The bf16-emulating adjoint chain (G_k = RNE(y_k), dH <- RNE(a_k y_k + dH), dH_0 =
    RNE(fl32(alpha dZ)) exactly) and the envelope of dH after K steps."""
    G = np.asarray(dZ, dtype=np.float32)
    dH = scaled_bf16(G, alpha)
    E_g, E_d = np.zeros(G.shape), np.zeros(G.shape)
    for k in range(K - 1, -1, -1):
        yw = alpha if k >= 1 else None
        t_d, d_d = backward_step_bf16(csr_t, G, dH, alpha, k, p_drop, seed)
        E_d = O.envelope(*csr_t, E_g, E_d, t_d, d_d, alpha, k, p_drop, seed, transposed=True,
                         h_weight=1.0, y_weight=yw)
        dH = O.round_bf16(t_d.astype(np.float32))
        if k >= 1:
            t_g, d_g = O.step_exact(*csr_t, G, None, alpha, k, p_drop, seed, transposed=True)
            E_g = O.envelope(*csr_t, E_g, None, t_g, d_g, alpha, k, p_drop, seed,
                             transposed=True)
            G = O.round_bf16(t_g.astype(np.float32))
    return dH, E_d


def within_envelope(out, ref, E, label=""):
    """Assert |out - ref| <= E elementwise; print the worst ratio and the bit-equal share."""
    out = np.asarray(out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    ratio = np.abs(out - ref) / E
    over = int((~(ratio <= 1.0)).sum())
    print(f"bf16 chain {label}: worst ratio {float(ratio.max()):.4f}, over the envelope {over} "
          f"of {out.size}, bit-equal to the emulated chain {100.0 * (out == ref).mean():.3f} %")
    assert over == 0, f"{over} of {out.size} elements outside the envelope {label}"


# ---------------------------------------------------------------------------------------
# device helpers (torch and the package are imported by the GPU modules only)
# ---------------------------------------------------------------------------------------

DEV = "cuda:0"


def torch_dtype(dtype):
    import torch

    return torch.float32 if dtype == "fp32" else torch.bfloat16


def operand(x, ld, dtype):
    """x [n, f] as the [:, :f] view of an [n, ld] device buffer whose padding is NaN (ld None:
    contiguous).  Returns (buffer, view)."""
    import torch

    src = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch_dtype(dtype))
    n, f = src.shape
    if ld is None:
        t = src.to(DEV)
        return t, t
    buf = torch.full((n, ld), float("nan"), dtype=src.dtype, device=DEV)
    buf[:, :f] = src.to(DEV)
    return buf, buf[:, :f]


def blank(n, f, ld, dtype):
    """An all-NaN output buffer [n, ld] and its [:, :f] view."""
    import torch

    buf = torch.full((n, ld if ld is not None else f), float("nan"), dtype=torch_dtype(dtype),
                     device=DEV)
    return buf, buf[:, :f]


def result(buf, f):
    """The values of an output buffer's view as fp64, after asserting that its padding is still
    NaN (not written) and that the result is finite (no padding read into it)."""
    import torch

    assert bool(torch.isnan(buf[:, f:]).all()), "output padding was written"
    out = buf[:, :f].float().cpu().numpy().astype(np.float64)
    assert np.isfinite(out).all(), "padding (NaN) or stale memory reached the result"
    return out


def randn(shape, seed, dtype):
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return O.round_bf16(x) if dtype == "bf16" else x


def csr_of(G, transpose=False):
    """(indptr, indices, w32) of the device graph's A_hat as numpy arrays (Graph.csr()), or of
    its transpose (the same fp32 values, rows sorted by column)."""
    rp, col, val, _ = G.csr()
    rp, col, val = rp.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
    if not transpose:
        return rp.astype(np.int64), col.astype(np.int64), val
    t = sp.csr_matrix((val, col, rp), shape=(G.rows, G.n)).T.tocsr()
    t.sort_indices()
    return t.indptr.astype(np.int64), t.indices.astype(np.int64), t.data


def check_last_rows(csr, n):
    """The last row of Zin is gathered by more rows than itself and the last held row has
    entries, so the piecewise last-row loads contribute to checked values."""
    indptr, indices, _ = csr
    assert indptr[-1] > indptr[-2], "the last held row has no entries"
    assert int((indices == n - 1).sum()) >= 2, "the last row of Zin has no neighbours"


def propagate_backward_views(G, dZ, dH, K, alpha, p_drop=0.0, seed=0):
    """appnp_propagate_bwd on the operands as given (``ppnp_amd.propagate_backward`` makes dZ
    contiguous first, which would drop the padded layout)."""
    import torch
    from ppnp_amd import _lib
    from ppnp_amd.ops import _DTYPES, _ld, _stream, _vp

    lib = _lib.load()
    dt = _DTYPES[dZ.dtype]
    f = int(dZ.shape[1])
    ws_bytes = int(lib.appnp_workspace_bytes(G.handle, f, _ld(dH), dt)) if K >= 2 else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=G.device) if ws_bytes else None
    with torch.cuda.device(G.device):
        rc = lib.appnp_propagate_bwd(G.handle, _vp(dZ), _ld(dZ), _vp(dH), _ld(dH), f, dt, int(K),
                                     float(alpha), float(p_drop), int(seed) & (2**64 - 1),
                                     _vp(ws), ws_bytes, _stream(G.device))
    _lib.check("appnp_propagate_bwd", rc)
    return dH
