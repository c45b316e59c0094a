"""GPU: bf16 storage, to the rounding.

The loose bf16 bar of tests/test_gpu_parity.py (2e-2 of the largest entry of the whole matrix)
passes a kernel that truncates instead of rounding to nearest-even, one that stores a wrong
value into a small element, and one that rotates a buffer wrongly at one parity of K.  Here every
element of one step must land within half a bf16 spacing of the exact step on the kernel's own
operands, plus an fp32 accumulation bound (oracle ``step_exact`` / ``close_bf16_step``), and
chains whose intermediates are not visible must stay inside the derived envelope around the
bf16-emulating chain (oracle ``envelope``).  No bound here is measured on a device; the share of
elements bit-equal to the rounded exact value is printed, not asserted.
"""

import numpy as np
import pytest
import torch

import step_variants as SV
from oracle import ppnp_oracle as O

pytestmark = pytest.mark.gpu


def _pa():
    import ppnp_amd

    return ppnp_amd


@pytest.fixture(scope="module")
def graphs():
    """(Graph, its A_hat as numpy CSR, the CSR the adjoint multiplies) by (name, mode)."""
    cache = {}

    def get(name, mode="sym"):
        if (name, mode) not in cache:
            pa = _pa()
            adj = SV.adjacency(name)
            directed = (adj != adj.T).nnz > 0
            G = pa.Graph.from_scipy(adj, mode=mode, device=SV.DEV,
                                    transpose=(mode == "rw" or directed))
            csr = SV.csr_of(G)
            self_adjoint = G.mode == "sym" and G.symmetric
            assert self_adjoint == (mode == "sym" and not directed)
            csr_t = csr if self_adjoint else SV.csr_of(G, transpose=True)
            if not directed:
                SV.check_last_rows(csr, G.n)
            cache[(name, mode)] = (G, csr, csr_t)
        return cache[(name, mode)]

    yield get
    for G, _, _ in cache.values():
        G.close()


def test_graph_shapes(graphs):
    n = SV.N_BIG
    for name in ("L1", "Bs", "Bsh", "Bl"):
        G, csr, _ = graphs(name)
        st = SV.stats(name)
        lens = np.diff(csr[0])
        assert (G.n, G.nnz_hat) == (st.n, st.nnz)
        assert int((lens > SV.K_HEAVY_ROW).sum()) == st.n_heavy
        assert int((lens > SV.K_HUB_ROW).sum()) == st.n_hub
    assert graphs("L1")[0].n == 4000 and SV.stats("L1").n_hub >= 1
    assert graphs("Bs")[0].nnz_hat < 24 * n and graphs("Bsh")[0].nnz_hat < 24 * n
    assert SV.stats("Bs").n_heavy == 0 and SV.stats("Bsh").n_heavy == 6
    assert graphs("Bl")[0].nnz_hat >= 24 * n


# ---------------------------------------------------------------------------------------
# 1. one step
# ---------------------------------------------------------------------------------------

WIDTHS = [1, 3, 8, 15, 16, 64, 100, 136]
PADDED_LD = {1: 8, 3: 8, 8: 16, 15: 16, 16: 24, 64: 72, 100: 104, 136: 144}
# (padded, mode, p_drop, k): each graph meets all eight, each width four of them, among them
# both layouts, both normalisations and both dropout settings (tests/test_step_variants.py)
COMBOS = [(pad, mode, p, k) for pad in (False, True) for mode in ("sym", "rw")
          for p, k in ((0.0, 0), (0.3, 3))]
STEP_CASES = [(g, f) + COMBOS[(i + 3 * j) % 8]
              for j, g in enumerate(("L1", "Bs", "Bsh", "Bl")) for i, f in enumerate(WIDTHS)]


@pytest.mark.parametrize("g,f,padded,mode,p_drop,k", STEP_CASES,
                         ids=[f"{c[0]}-F{c[1]}-{'padded' if c[2] else 'contiguous'}-{c[3]}-p{c[4]}"
                              for c in STEP_CASES])
def test_single_step(graphs, g, f, padded, mode, p_drop, k):
    pa = _pa()
    G, csr, _ = graphs(g, mode)
    ld = PADDED_LD[f] if padded else None
    z = SV.randn((G.n, f), f * 17 + k, "bf16")
    h = SV.randn((G.n, f), f * 17 + k + 1, "bf16")
    _, Zin = SV.operand(z, ld, "bf16")
    _, H = SV.operand(h, ld, "bf16")
    buf, out = SV.blank(G.n, f, ld, "bf16")
    alpha = 0.1 if k == 0 else 0.2
    pa.step(G, Zin, H, out, k, alpha, p_drop=p_drop, seed=77)
    t, delta = O.step_exact(*csr, z, h, alpha, k, p_drop, 77)
    O.close_bf16_step(SV.result(buf, f), t, delta, f"{g} F={f} ld={ld} {mode} p={p_drop}")


# ---------------------------------------------------------------------------------------
# 2. forward induction: every iterate of a K-step call against the exact step on the kernel's
#    own previous iterate
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("g,f,ld,alpha", [("Md", 15, None, 0.2), ("L1", 100, 104, 0.1),
                                          ("Bl", 100, None, 0.1)],
                         ids=["msacad-F15", "L1-F100-ld104", "Bl-F100"])
def test_forward_induction(graphs, g, f, ld, alpha):
    pa = _pa()
    G, csr, _ = graphs(g)
    h = SV.randn((G.n, f), f + 5, "bf16")
    _, H = SV.operand(h, ld, "bf16")
    Z = []
    for K in range(5):
        buf, out = SV.blank(G.n, f, ld, "bf16")
        pa.propagate_forward(G, H, K, alpha, out=out)
        SV.result(buf, f)
        Z.append(out)
    assert torch.equal(Z[0], H)
    # iterate k of a K-step call is bitwise the k-step call's result: the same instantiation and
    # input bits, only the internal buffer's leading dimension differs.  Asserted by chaining
    # single steps on operands of the same alignment.
    cur = H
    for K in range(1, 5):
        _, nxt = SV.blank(G.n, f, ld, "bf16")
        pa.step(G, cur, H, nxt, K - 1, alpha)
        assert torch.equal(nxt, Z[K]), f"the {K}-step call is not {K} chained steps"
        cur = nxt
    for K in range(1, 5):
        prev = Z[K - 1].float().cpu().numpy()
        t, delta = O.step_exact(*csr, prev, h, alpha, K - 1, 0.0, 0)
        O.close_bf16_step(Z[K].float().cpu().numpy(), t, delta, f"{g} F={f} Z_{K}")


# ---------------------------------------------------------------------------------------
# 3. backward, K = 1: dH = RNE(1 y + RNE(fl32(alpha dZ)))
# ---------------------------------------------------------------------------------------

BWD_GRAPHS = [("L1", "sym", 100, 104), ("Bs", "sym", 15, None), ("L1", "rw", 16, None),
              ("D", "sym", 6, 8), ("D", "rw", 13, 16)]


@pytest.mark.parametrize("g,mode,f,ld", BWD_GRAPHS,
                         ids=[f"{g}-{m}-F{f}-ld{ld}" for g, m, f, ld in BWD_GRAPHS])
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
def test_backward_one_step(graphs, g, mode, f, ld, p_drop):
    G, _, csr_t = graphs(g, mode)
    dz = SV.randn((G.n, f), f + 11, "bf16")
    _, dZ = SV.operand(dz, ld, "bf16")
    buf, dH = SV.blank(G.n, f, ld, "bf16")
    SV.propagate_backward_views(G, dZ, dH, 1, 0.1, p_drop, 8)
    t, delta = SV.backward_step_bf16(csr_t, dz, SV.scaled_bf16(dz, 0.1), 0.1, 0, p_drop, 8)
    O.close_bf16_step(SV.result(buf, f), t, delta, f"bwd K=1 {g} {mode} F={f} p={p_drop}")


# ---------------------------------------------------------------------------------------
# 4. backward, K = 2 and 3: the envelope around the bf16-emulating chain (both parities of the
#    buffer rotation)
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("g,mode,f,ld", [("L1", "sym", 15, 16), ("D", "sym", 6, None),
                                         ("L1", "rw", 20, None), ("Bs", "sym", 9, 16)],
                         ids=["L1-sym-F15-ld16", "D-sym-F6", "L1-rw-F20", "Bs-sym-F9-ld16"])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
def test_backward_chain(graphs, g, mode, f, ld, K, p_drop):
    G, _, csr_t = graphs(g, mode)
    dz = SV.randn((G.n, f), f + 13, "bf16")
    _, dZ = SV.operand(dz, ld, "bf16")
    buf, dH = SV.blank(G.n, f, ld, "bf16")
    SV.propagate_backward_views(G, dZ, dH, K, 0.1, p_drop, 8)
    ref, E = SV.backward_chain_bf16(csr_t, dz, K, 0.1, p_drop, 8)
    SV.within_envelope(SV.result(buf, f), ref, E, f"bwd K={K} {g} {mode} F={f} p={p_drop}")
