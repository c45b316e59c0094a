"""Which instantiation of the fused step kernel a call reaches, and a table of cases that reaches
every vector-tail cell of it.  A plain module shared by tests/test_step_variants.py (CPU: the
table covers the cells), tests/test_gpu_vector_tails.py and tests/test_gpu_bf16_exact.py.

The vector-tail code of ppnp_amd/csrc/appnp_spmm.hip (the TAIL switches of frag_load /
frag_store, the piecewise read of a buffer's last row) runs only when F is not a multiple of V,
every leading dimension is a multiple of V, and launch_step keeps that V.  ``expected_variant``
mirrors those decisions on the host; ``CASES`` names, per cell (dtype, V, F mod V), a graph, a
width and a layout that lands in it.  profiles/step_variants_hit.txt records the instantiations
a kernel trace of the GPU modules saw, checked once against ``expected_kernel`` over CASES.

``expected_grid`` mirrors the grid of launch_step (the block cap, the heavy blocks of a narrow
launch), and the OVERRIDE_* tables name the cases that tests/override_worker.py runs under the
tuning overrides (tests/test_gpu_overrides.py; their reach is proved on the host in
tests/test_step_variants.py, their kernels and grids traced in profiles/override_paths_hit.txt).
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
K_WAVES_PER_BLOCK = 4   # kBlock / kWave
K_MAX_BLOCKS = 1 << 22  # launch_step's cap on gridDim.x (APPNP_MAX_BLOCKS lowers it)
K_HEAVY_BLOCKS = 4096   # most heavy-row blocks a narrow launch appends


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


def expected_kernel(dtype, epi, variant, nnz, nnz_rows, n_rows, n_heavy, uw=None, un=None):
    """The instantiation's name as a kernel trace prints it, k_step_wide / k_step_narrow
    <T, V, G, EPI, U, TAIL>: U mirrors ``uw`` / ``un`` of launch_step and launch_g.  ``uw`` /
    ``un``: the APPNP_UW / APPNP_UN overrides (launch_g runs U = 1 for a uw that is none of 2, 4,
    8, and the narrow U = 8 only at V <= 2)."""
    V, G, wide, rem, regime = variant
    latency = regime == "latency"
    long_rows = nnz >= K_WIDE_AVG_ROW * n_rows
    long_whole = (nnz_rows or nnz) >= K_WIDE_AVG_ROW * n_rows
    if wide:
        if uw is None:
            uw = (8 if (latency and n_heavy > 0)
                  else 2 if (not latency and (long_rows or long_whole)) else 1)
        U = uw if uw in (2, 4, 8) else 1
    else:
        if un is None:
            un = 8 if latency else 4
        U = 8 if (un == 8 and V <= 2) else 4
    T = "float" if dtype == "fp32" else "unsigned short"
    return (f"k_step_{'wide' if wide else 'narrow'}<{T}, {V}, {G}, {EPI[epi]}, {U}, "
            f"{'true' if rem else 'false'}>")


def rows_per_block(variant):
    """Rows a block of the launch takes per trip of its grid-stride loop: a wave per row (wide),
    or 64 / G rows per wave (narrow)."""
    _, G, wide, _, _ = variant
    return K_WAVES_PER_BLOCK if wide else K_WAVES_PER_BLOCK * (K_WAVE // G)


def slabs_of(variant, f):
    V, G = variant[0], variant[1]
    return (f + G * V - 1) // (G * V)


def uncapped_blocks(variant, n_rows, n_hub):
    """gridDim.x of the row pass before the cap: the hub rows count as virtual rows of a wide
    launch only."""
    rpb = rows_per_block(variant)
    return (n_rows + (n_hub if variant[2] else 0) + rpb - 1) // rpb


def expected_grid(variant, n_rows, n_hub, n_heavy, max_blocks=K_MAX_BLOCKS, *, f):
    """(light_blocks, heavy_blocks, slabs) of launch_step's grid for ``f`` features: gridDim.x =
    light_blocks + heavy_blocks, gridDim.y = slabs.  The hub list is dropped unless the launch
    is wide, the heavy list unless it is narrow; the cap binds the row pass only."""
    wide = variant[2]
    light = min(uncapped_blocks(variant, n_rows, n_hub), min(max_blocks, K_MAX_BLOCKS))
    heavy = 0
    if not wide and n_heavy > 0:
        heavy = min((n_heavy + K_WAVES_PER_BLOCK - 1) // K_WAVES_PER_BLOCK, K_HEAVY_BLOCKS)
    return light, heavy, slabs_of(variant, f)


# ---------------------------------------------------------------------------------------
# graphs (seeded; the shapes are asserted in tests/test_step_variants.py)
# ---------------------------------------------------------------------------------------

N_BIG = 66_000
BH_N, BH_HEAVY, BH_FAN, BH_MUL = 100_000, 17_000, 33, 7919
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
    the range.  Md: MS-Academic-sized.  D: directed (upper triangle).  Dh: directed, bandwidth
    regime: the upper triangle of Bs plus edges INTO six nodes (40 .. 600 each), so A_hat^T, which
    the adjoint multiplies, has six heavy rows and a hub row (12 345) while A_hat has neither.  Bh: 17 000 heavy rows of
    34 entries (more than the 16 384 waves of a narrow launch's heavy blocks) among short ones;
    no RNG: node h < 17 000 is joined to 17 000 + ((33 h + t) 7919 mod 83 000), t = 0..32, and
    7919 is coprime to 83 000, so the 561 000 edges are distinct and spread evenly."""
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
    if name == "Bh":
        rest = BH_N - BH_HEAVY
        h = np.repeat(np.arange(BH_HEAVY, dtype=np.int64), BH_FAN)
        t = np.tile(np.arange(BH_FAN, dtype=np.int64), BH_HEAVY)
        dst = BH_HEAVY + ((BH_FAN * h + t) * BH_MUL) % rest
        half = sp.coo_matrix((np.ones(h.size, np.float32), (h, dst)), shape=(BH_N, BH_N)).tocsr()
        a = (half + half.T).tocsr().astype(np.float32)
        a.sort_indices()
        return a
    if name == "Dh":
        rng = np.random.default_rng(37)
        into = [7, 4099, 30_000, 47_111, N_BIG - 1, 12_345]
        counts = [40, 45, 50, 55, 60, 600]
        src = np.concatenate([rng.choice(N_BIG, c, replace=False) for c in counts])
        dst = np.repeat(into, counts)
        extra = sp.coo_matrix((np.ones(len(src), np.float32), (src, dst)),
                              shape=(N_BIG, N_BIG)).tocsr()
        a = ((sp.triu(adjacency("Bs"), format="csr") + extra) > 0).astype(np.float32).tocsr()
        a.setdiag(0)
        a.eliminate_zeros()
        a.sort_indices()
        return a
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


# ---------------------------------------------------------------------------------------
# the cases of tests/override_worker.py (tests/test_gpu_overrides.py runs them)
# ---------------------------------------------------------------------------------------

# op: "fwd" (propagate_forward) / "bwd" (appnp_propagate_bwd on the views as given); ld None:
# contiguous; mode / transpose: how the device graph is built
OCase = namedtuple("OCase", "graph dtype f ld op K p_drop mode transpose",
                   defaults=("fwd", 2, 0.0, "sym", False))
# appnp_spmm on the 900 x 700 CSR of tests/test_gpu_parity.py::test_spmm_matches_dense
SpmmCase = namedtuple("SpmmCase", "f p_drop transposed_key", defaults=(0.0, False))

O_ALPHA, O_SEED = 0.1, 41
DIRECTED = ("D", "Dh")
SPMM_ROWS, SPMM_COLS, SPMM_DENSITY = 900, 700, 0.02

# grid-stride loops: APPNP_MAX_BLOCKS = 1 and 7 (K = 2)
OVERRIDE_CAPPED = [
    OCase("L1", "fp32", 100, 104), OCase("L1", "fp32", 100, 104, "bwd"),
    OCase("L1", "fp32", 7, 10), OCase("L1", "bf16", 13, 20, p_drop=0.3),
    OCase("Bsh", "fp32", 7, 10), OCase("Bsh", "fp32", 7, 10, "bwd"),
    OCase("Bsh", "bf16", 13, 20), OCase("Bsh", "fp32", 66, 68),
    # the adjoint accumulates into dH, so a hub row computed twice shows in the value -- when the
    # two computations fall into different trips: Bsh's hub row is row 12 345 (L1's is row 0,
    # whose regular-pass turn comes in the same trip as its hub-first turn)
    OCase("Bsh", "fp32", 66, 68, "bwd"),
    OCase("Bs", "fp32", 13, 16),
    OCase("D", "fp32", 16, None, mode="rw", transpose=True),
    OCase("D", "fp32", 16, None, "bwd", mode="rw", transpose=True),
    # D has no heavy and no hub row, in A_hat or in A_hat^T: it is the no-list case of the
    # transposed CSR.  Dh's adjoint runs on an A_hat^T with six heavy rows and a hub row: the
    # narrow launch appends heavy blocks for t_heavy, the wide one dispatches t_hub first
    OCase("Dh", "fp32", 7, 10, "bwd", mode="rw", transpose=True),
    OCase("Dh", "fp32", 66, 68, "bwd", mode="rw", transpose=True),
    SpmmCase(130), SpmmCase(7), SpmmCase(130, 0.5, True),
]
# more heavy rows than the heavy blocks have waves: no override needed (and with the cap of 7,
# both loops of the narrow kernel iterate in one launch)
OVERRIDE_BH = [OCase("Bh", "fp32", 7, 8), OCase("Bh", "fp32", 7, 8, "bwd"),
               OCase("Bh", "bf16", 13, 16)]
# entries in flight and cache policy: APPNP_UW = 4, APPNP_UN = 4, APPNP_NT = 7.  The last case
# is the narrow launch of the latency regime, the only one whose U (8) APPNP_UN = 4 changes.
OVERRIDE_UNROLL = [
    OCase("L1", "fp32", 100, 104, K=3), OCase("L1", "bf16", 100, 104, K=3),
    OCase("L1", "fp32", 100, 104, "bwd"), OCase("L1", "bf16", 100, 104, "bwd"),
    OCase("Bl", "fp32", 13, 16, K=3), OCase("Bs", "fp32", 13, 16, K=3),
    OCase("Bs", "bf16", 9, 16, K=3), OCase("Md", "bf16", 15, None, K=3),
    OCase("Md", "fp32", 7, None, K=3),
]

OVERRIDE_SETS = {"capped": OVERRIDE_CAPPED, "capped-bh": OVERRIDE_CAPPED + OVERRIDE_BH,
                 "bh": OVERRIDE_BH, "unroll": OVERRIDE_UNROLL}


def ocase_id(c):
    if isinstance(c, SpmmCase):
        return f"spmm-F{c.f}" + ("-drop" if c.p_drop else "") + ("-tkey" if c.transposed_key else "")
    return (f"{c.graph}-{c.mode}-{c.dtype}-F{c.f}-ld{c.ld or c.f}-{c.op}-K{c.K}"
            + ("-drop" if c.p_drop else ""))


def ocase_seed(c):
    if isinstance(c, SpmmCase):
        return c.f * 131 + (5 if c.p_drop else 0)
    return c.f * 131 + (c.ld or c.f) + (7 if c.op == "bwd" else 0)


def spmm_matrix():
    from test_gpu_parity import _rand_csr

    return _rand_csr(SPMM_ROWS, SPMM_COLS, SPMM_DENSITY, 130)


@functools.lru_cache(maxsize=None)
def ostats(graph, mode="sym", transposed=False):
    """``stats`` for any normalisation, and of A_hat^T (the CSR an adjoint multiplies when A_hat
    is not symmetric)."""
    ah = a_hat(graph, mode)
    if transposed:
        ah = ah.T.tocsr()
    lens = np.diff(ah.indptr)
    n = ah.shape[0]
    return Stats(n, n, int(ah.nnz), int((lens > K_HEAVY_ROW).sum()), int((lens > K_HUB_ROW).sum()))


def ocase_launch(c):
    """(epi, lds, Stats, nnz known to the host) of the step launches of an override case."""
    if isinstance(c, SpmmCase):  # appnp_spmm: no row lists, nnz unknown (-1) on the host
        st = Stats(SPMM_COLS, SPMM_ROWS, -1, 0, 0)
        return "PARTIAL", (c.f, c.f), st
    ld = c.ld or c.f
    self_adjoint = c.mode == "sym" and c.graph not in DIRECTED
    st = ostats(c.graph, c.mode, c.op == "bwd" and not self_adjoint)
    return ("FWD" if c.op == "fwd" else "BWD"), (ld, ld, line_ld(c.f, c.dtype)), st


def ocase_variant(c):
    epi, lds, st = ocase_launch(c)
    dtype = "fp32" if isinstance(c, SpmmCase) else c.dtype
    return expected_variant(dtype, c.f, lds, st.rows, st.nnz, st.n_heavy, st.n_hub)


def ocase_prediction(c, max_blocks=K_MAX_BLOCKS, uw=None, un=None):
    """(kernel name, (gridDim.x, gridDim.y)) of every step launch of the case."""
    epi, lds, st = ocase_launch(c)
    dtype = "fp32" if isinstance(c, SpmmCase) else c.dtype
    v = ocase_variant(c)
    light, heavy, slabs = expected_grid(v, st.rows, st.n_hub, st.n_heavy, max_blocks, f=c.f)
    return (expected_kernel(dtype, epi, v, st.nnz, 0, st.rows, st.n_heavy, uw, un),
            (light + heavy, slabs))


# the remainder pass with many source blocks: APPNP_SB_ROWS = 1024 on a 66 000-node graph
SB_N, SB_EDGES, SB_HUB, SB_ROWS, SB_NB = N_BIG, 4 * N_BIG, 3000, 1024, 65
SbCase = namedtuple("SbCase", "width f op p_drop", defaults=("fwd", 0.0))
SB_K = 3
SB_CASES = [
    SbCase(4, 100), SbCase(4, 36), SbCase(4, 33), SbCase(4, 3), SbCase(4, 36, p_drop=0.25),
    SbCase(4, 100, "bwd"),
    SbCase(8, 40), SbCase(8, 37), SbCase(8, 5), SbCase(8, 40, p_drop=0.25), SbCase(8, 40, "bwd"),
    SbCase(16, 13), SbCase(16, 13, "bwd"),
]
# (name, weighted, mode per width): the unit graph stores no values in the copy; the weighted
# one (values 0.5, 1, 2) keeps them, and its W8 copy is normalised 'rw' (no split adjoint there:
# A_hat is not symmetric)
SB_GRAPHS = [("unit", False, {4: "sym", 8: "sym", 16: "sym"}),
             ("weighted", True, {4: "sym", 8: "rw", 16: "sym"})]
SB_FEATURES = {4: 100, 8: 40, 16: 13}  # the width Graph.from_scipy lays the copy out for


def sb_case_id(gname, c):
    return f"{gname}-W{c.width}-F{c.f}-{c.op}" + ("-drop" if c.p_drop else "")


def sb_cases_of(gname):
    modes = dict((g[0], g[2]) for g in SB_GRAPHS)[gname]
    return [c for c in SB_CASES if not (c.op == "bwd" and modes[c.width] != "sym")]


@functools.lru_cache(maxsize=None)
def sb_adjacency(weighted):
    """O.synth_graph(66 000, 264 000) plus one hub row of 3000 entries, as the ``adj`` fixture of
    tests/test_gpu_split.py builds it; ``weighted``: symmetric values drawn from 0.5, 1, 2."""
    a = O.synth_graph(SB_N, SB_EDGES, seed=5).tolil()
    rng = np.random.default_rng(6)
    hub = rng.choice(np.arange(1, SB_N), size=SB_HUB, replace=False)
    a[0, hub] = 1.0
    a[hub, 0] = 1.0
    a = sp.csr_matrix(a, dtype=np.float32)
    if weighted:
        up = sp.triu(a, k=1, format="csr").astype(np.float32)
        up.data = np.random.default_rng(7).choice(np.float32([0.5, 1.0, 2.0]), size=up.nnz)
        a = (up + up.T).tocsr().astype(np.float32)
    a.sort_indices()
    return a


def pad4(f):
    return (f + 3) // 4 * 4
