"""GPU: the vector-tail code of the step kernels (appnp_spmm.hip: the TAIL switches of frag_load /
frag_store and the piecewise read of a buffer's last row) at V >= 4, in every epilogue.

Every entry of tests/step_variants.py CASES -- tests/test_step_variants.py shows that together
they reach each (dtype, V, F mod V) cell in a wave-per-row and in a narrow-row launch -- runs on
operands that are [:, :F] views of [n, ld] buffers whose padding is NaN.  After the run the
output's padding must still be NaN (a tail store wrote exactly F mod V elements), the result
finite (no padding element, which a full-vector read of a tail fragment does load, reached a
stored value) and equal to the reference:

  fp32  the module-wide fp32 bar of tests/test_gpu_parity.py (close_fp32) against the fp64 oracle
  bf16  single steps: within half a bf16 spacing plus the fp32 accumulation bound of the exact
        step on the kernel's own operands, for every element (oracle close_bf16_step); chains:
        the derived envelope around the bf16-emulating chain (oracle envelope)

The Chebyshev epilogue's cells run in tests/test_gpu_solve.py (ld104 cases).
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import step_variants as SV
from oracle import ppnp_oracle as O
from test_gpu_parity import close_fp32

pytestmark = pytest.mark.gpu

ALPHA, STEP_K, SEED = 0.1, 2, 41


def _pa():
    import ppnp_amd

    return ppnp_amd


@pytest.fixture(scope="module")
def graphs():
    """Device graphs by name, built on first use; with them their A_hat as the device holds it
    (int64 indptr / indices, fp32 values).  The shapes the names promise are asserted."""
    cache = {}

    def get(name):
        if name not in cache:
            pa = _pa()
            st = SV.stats(name)
            if name == "R":
                G = pa.Graph.from_scipy(SV.adjacency("R"), device=SV.DEV, row_lo=SV.ROWS_LO,
                                        row_hi=SV.ROWS_HI, split_local=True)
                pa.ops.shard_offsets(G, SV.ROWS_SHARDS, SV.ROWS_SHARD_ROWS)
            else:
                G = pa.Graph.from_scipy(SV.adjacency(name), device=SV.DEV)
            assert (G.n, G.rows, G.nnz_hat) == (st.n, st.rows, st.nnz)
            csr = SV.csr_of(G)
            lens = np.diff(csr[0])
            assert int((lens > SV.K_HEAVY_ROW).sum()) == st.n_heavy
            assert int((lens > SV.K_HUB_ROW).sum()) == st.n_hub
            if name != "R":
                SV.check_last_rows(csr, G.n)
            cache[name] = (G, csr)
        return cache[name]

    yield get
    for G, _ in cache.values():
        G.close()


def _masked(name, p_drop, k=STEP_K):
    ah = SV.a_hat(name)
    return O.masked_operator(ah, k, p_drop, SEED) if p_drop > 0 else ah


def _case_seed(c):
    return c.f * 131 + c.ld


# ---------------------------------------------------------------------------------------
# one forward step
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", [c for c in SV.CASES if c.epi == "FWD"], ids=SV.case_id)
def test_forward_step(graphs, c):
    pa = _pa()
    G, csr = graphs(c.graph)
    v = SV.case_variants(c)[0][1]
    assert v[3] == c.f % v[0] and v[3] > 0
    n = G.n
    z = SV.randn((n, c.f), _case_seed(c), c.dtype)
    h = SV.randn((n, c.f), _case_seed(c) + 1, c.dtype)
    _, Zin = SV.operand(z, c.ld, c.dtype)
    _, H = SV.operand(h, c.ld, c.dtype)
    buf, out = SV.blank(n, c.f, c.ld, c.dtype)
    pa.step(G, Zin, H, out, STEP_K, ALPHA, p_drop=c.p_drop, seed=SEED)
    got = SV.result(buf, c.f)
    if c.dtype == "fp32":
        close_fp32(got, (1.0 - ALPHA) * (_masked(c.graph, c.p_drop) @ z.astype(np.float64))
                   + ALPHA * h.astype(np.float64))
    else:
        t, delta = O.step_exact(*csr, z, h, ALPHA, STEP_K, c.p_drop, SEED)
        O.close_bf16_step(got, t, delta, SV.case_id(c))


# ---------------------------------------------------------------------------------------
# the adjoint, K = 1 and K = 2 (K = 2 also gathers from the internal buffer)
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", [c for c in SV.CASES if c.epi == "BWD"], ids=SV.case_id)
def test_backward(graphs, c):
    G, csr = graphs(c.graph)
    v = SV.case_variants(c)[0][1]
    assert v[3] == c.f % v[0] and v[3] > 0
    n = G.n
    dz = SV.randn((n, c.f), _case_seed(c) + 2, c.dtype)
    _, dZ = SV.operand(dz, c.ld, c.dtype)
    for K in (1, 2):
        buf, dH = SV.blank(n, c.f, c.ld, c.dtype)
        SV.propagate_backward_views(G, dZ, dH, K, ALPHA, c.p_drop, SEED)
        got = SV.result(buf, c.f)
        label = f"{SV.case_id(c)} K={K}"
        if c.dtype == "fp32":
            close_fp32(got, O.appnp_backward(SV.a_hat(c.graph), dz, K, ALPHA, c.p_drop, SEED))
        elif K == 1:
            t, delta = SV.backward_step_bf16(csr, dz, SV.scaled_bf16(dz, ALPHA), ALPHA, 0,
                                             c.p_drop, SEED)
            O.close_bf16_step(got, t, delta, label)
        else:
            ref, E = SV.backward_chain_bf16(csr, dz, K, ALPHA, c.p_drop, SEED)
            SV.within_envelope(got, ref, E, label)


# ---------------------------------------------------------------------------------------
# the fp32 partial chain of a row-partitioned step: PARTIAL, FINISH, ACCUM
# ---------------------------------------------------------------------------------------


def _held(c, cols=None):
    """fp64 (masked) A_hat rows [ROWS_LO, ROWS_HI), restricted to the column range ``cols``."""
    m = _masked("R", c.p_drop)[SV.ROWS_LO:SV.ROWS_HI].tocsc()
    if cols is not None:
        keep = np.zeros(SV.ROWS_N, dtype=bool)
        for lo, hi in cols:
            keep[lo:hi] = True
        m = m @ sp.diags(keep.astype(np.float64))
    return m.tocsr()


@pytest.mark.parametrize("c", [c for c in SV.CASES if c.epi in ("PARTIAL", "FINISH", "ACCUM")],
                         ids=SV.case_id)
def test_partial_chain(graphs, c):
    from ppnp_amd import _lib as L

    pa = _pa()
    G, _ = graphs("R")
    for _, v, _ in SV.case_variants(c):
        assert v[0] == 4 and v[3] == c.f % 4 and v[3] > 0
    lo, hi, n, rows = SV.ROWS_LO, SV.ROWS_HI, SV.ROWS_N, SV.ROWS_HI - SV.ROWS_LO
    sr = SV.ROWS_SHARD_ROWS
    s = 1.0 - ALPHA
    z = SV.randn((n, c.f), _case_seed(c), "fp32")
    h = SV.randn((rows, c.f), _case_seed(c) + 1, "fp32")
    part = SV.randn((rows, c.f), _case_seed(c) + 2, "fp32")
    z64 = z.astype(np.float64)
    _, Zin = SV.operand(z, c.ld, "fp32")
    _, H = SV.operand(h, c.ld, "fp32")
    kw = dict(p_drop=c.p_drop, seed=SEED)
    if c.epi == "PARTIAL":
        buf, P = SV.blank(rows, c.f, c.ld_p, "fp32")
        pa.step(G, Zin, None, P, STEP_K, ALPHA, part=L.PART_LOCAL, **kw)
        close_fp32(SV.result(buf, c.f), s * (_held(c, [(lo, hi)]) @ z64))
        # the last shard's columns reach the last row of Zin
        buf, P = SV.blank(rows, c.f, c.ld_p, "fp32")
        pa.ops.step_shards(G, 2, 3, L.SHARDS_FIRST, Zin, None, None, P, STEP_K, ALPHA, **kw)
        close_fp32(SV.result(buf, c.f), s * (_held(c, [(2 * sr, n)]) @ z64))
    elif c.epi == "FINISH":
        pbuf, P = SV.operand(part, c.ld_p, "fp32")
        buf, out = SV.blank(rows, c.f, c.ld, "fp32")
        pa.step(G, Zin, H, out, STEP_K, ALPHA, part=L.PART_REMOTE, partial=P, **kw)
        ref = s * (_held(c, [(0, lo), (hi, n)]) @ z64) + part + ALPHA * h.astype(np.float64)
        close_fp32(SV.result(buf, c.f), ref)
        assert torch.equal(P.cpu(), torch.from_numpy(part))  # the partial is read only
    else:  # ACCUM: partial += the product over shards [1, 3)
        pbuf, P = SV.operand(part, c.ld_p, "fp32")
        pa.ops.step_shards(G, 1, 3, L.SHARDS_ACC, Zin, None, None, P, STEP_K, ALPHA, **kw)
        close_fp32(SV.result(pbuf, c.f), part + s * (_held(c, [(sr, n)]) @ z64))


# ---------------------------------------------------------------------------------------
# K = 3 through appnp_propagate on padded views: the internal buffer as gather source
# ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("g,dtype,f,ld", SV.FORWARD_K3,
                         ids=[f"{g}-{d}-F{f}-ld{ld}" for g, d, f, ld in SV.FORWARD_K3])
def test_forward_three_steps(graphs, g, dtype, f, ld):
    pa = _pa()
    G, csr = graphs(g)
    h = SV.randn((G.n, f), f * 7 + ld, dtype)
    _, H = SV.operand(h, ld, dtype)
    buf, out = SV.blank(G.n, f, ld, dtype)
    p_drop = 0.3 if dtype == "bf16" and f == 13 else 0.0
    pa.propagate_forward(G, H, 3, ALPHA, p_drop=p_drop, seed=SEED, out=out)
    got = SV.result(buf, f)
    if dtype == "fp32":
        close_fp32(got, O.appnp_propagate(SV.a_hat(g), h, 3, ALPHA, p_drop, SEED))
    else:
        ref, E = SV.forward_chain_bf16(csr, h, 3, ALPHA, p_drop, SEED)
        SV.within_envelope(got, ref, E, f"{g} F={f} ld={ld} K=3")
