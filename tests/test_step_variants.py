"""CPU: the table of tests/step_variants.py reaches every vector-tail cell of the step kernels.

``expected_variant`` (the host mirror of pick_vec and launch_step) runs over ``CASES`` with
host-only graph statistics.  The GPU modules then run those cases; the mirror itself was
anchored once against a kernel trace (profiles/step_variants_hit.txt)."""

import numpy as np
import pytest

import step_variants as SV

FP32_CELLS = {("fp32", 2, 1), ("fp32", 4, 1), ("fp32", 4, 2), ("fp32", 4, 3)}
BF16_CELLS = ({("bf16", 2, 1)} | {("bf16", 4, r) for r in (1, 2, 3)}
              | {("bf16", 8, r) for r in range(1, 8)})
CELLS = FP32_CELLS | BF16_CELLS


def _cells(epi, keep=lambda case, variant, st: True):
    out = set()
    for c in SV.CASES:
        if c.epi != epi:
            continue
        for e, v, st in SV.case_variants(c):
            if v[3] and keep(c, v, st):
                out.add((c.dtype, v[0], v[3]))
    return out


def test_graph_shapes():
    n = SV.N_BIG
    l1, bs, bsh, bl = (SV.stats(g) for g in ("L1", "Bs", "Bsh", "Bl"))
    assert l1.n == 4000 and l1.n_heavy >= 3 and l1.n_hub >= 1
    assert bs.n == n and bs.nnz < 24 * n and bs.n_heavy == 0 and bs.n_hub == 0
    assert bsh.n == n and bsh.nnz < 24 * n and bsh.n_heavy == 6 and bsh.n_hub == 1
    assert bl.n == n and bl.nnz >= 24 * n
    assert min(l1.n, 1 << 16) == l1.n and n > 1 << 16  # latency / bandwidth regimes
    r = SV.stats("R")
    assert (r.n, r.rows, r.n_heavy) == (SV.ROWS_N, SV.ROWS_HI - SV.ROWS_LO, 0)
    assert SV.ROWS_SHARDS * SV.ROWS_SHARD_ROWS >= SV.ROWS_N
    md = SV.stats("Md")
    assert md.n == 18333 and md.n_heavy == 0
    # the last row of Zin is gathered by other rows and the last held row has entries, in every
    # part that a case multiplies
    for g in ("L1", "Bs", "Bsh", "Bl", "Md"):
        ah = SV.a_hat(g)
        SV.check_last_rows((ah.indptr, ah.indices, ah.data), ah.shape[0])
    held = SV.a_hat("R")[SV.ROWS_LO:SV.ROWS_HI]
    last = held[-1].indices
    assert SV.ROWS_N - 1 in last and (last < SV.ROWS_LO).any()          # REMOTE, shards 1-2
    assert ((last >= SV.ROWS_LO) & (last < SV.ROWS_HI)).any()           # LOCAL: the self loop
    assert (last >= 2 * SV.ROWS_SHARD_ROWS).any()                       # the last shard


def test_every_cell_forward_wave_row_and_narrow():
    wave = _cells("FWD", lambda c, v, st: SV.runs_wave_row(v, st.n_heavy))
    wide = _cells("FWD", lambda c, v, st: v[2])
    narrow = _cells("FWD", lambda c, v, st: not v[2] and v[1] <= 8 and c.graph in ("Bs", "Bsh"))
    assert wave == CELLS, sorted(CELLS - wave)
    assert wide == CELLS, sorted(CELLS - wide)
    assert narrow == CELLS, sorted(CELLS - narrow)
    # heavy rows inside a narrow launch too
    inside = _cells("FWD", lambda c, v, st: not v[2] and st.n_heavy > 0)
    assert {dt for dt, _, _ in inside} == {"fp32", "bf16"}
    # both regimes, and more than one row slab (F > 64 V)
    assert {v[4] for c in SV.CASES for _, v, _ in SV.case_variants(c)} == {"latency", "bandwidth"}
    assert any(c.f > 64 * v[0] and v[3] for c in SV.CASES for _, v, _ in SV.case_variants(c))


def test_every_cell_backward():
    got = _cells("BWD")
    assert got == CELLS, sorted(CELLS - got)


@pytest.mark.parametrize("epi", ["PARTIAL", "FINISH", "ACCUM"])
def test_fp32_cells_of_the_partial_chain(epi):
    want = {("fp32", 4, r) for r in (1, 2, 3)}
    got = _cells(epi)
    assert want <= got, sorted(want - got)
    for c in SV.CASES:
        if c.epi == epi:
            assert c.ld_p != c.ld and c.ld_p % 4 == 0  # the partial's own leading dimension


def test_cheb_cells_are_in_the_solve_module():
    """CHEB runs in tests/test_gpu_solve.py on its latency-regime hub graph (heavy rows keep
    V = 4): F = 101, 98, 99 in rows of 104 floats."""
    import test_gpu_solve as TS

    want = {("fp32", 4, 1), ("fp32", 4, 2), ("fp32", 4, 3)}
    got = set()
    for f, layout in TS.CASES:
        if layout == "ld104":
            v = SV.expected_variant("fp32", f, (104, 104, SV.line_ld(f, "fp32")), 2811, 20_000, 5, 1)
            if v[3]:
                got.add(("fp32", v[0], v[3]))
    assert want <= got


def test_bf16_single_step_cases_cover_the_combinations():
    """tests/test_gpu_bf16_exact.py::test_single_step: every graph meets all eight (layout,
    normalisation, dropout) combinations, every width both values of each."""
    import test_gpu_bf16_exact as TB

    for g in ("L1", "Bs", "Bsh", "Bl"):
        assert {c[2:] for c in TB.STEP_CASES if c[0] == g} == set(TB.COMBOS)
    for f in TB.WIDTHS:
        mine = [c for c in TB.STEP_CASES if c[1] == f]
        assert {c[2] for c in mine} == {False, True}
        assert {c[3] for c in mine} == {"sym", "rw"}
        assert {(c[4], c[5]) for c in mine} == {(0.0, 0), (0.3, 3)}


def test_a_third_of_the_cases_drop_edges():
    drop = sum(1 for c in SV.CASES if c.p_drop > 0)
    assert abs(drop - len(SV.CASES) / 3) <= 2
    assert len({SV.case_id(c) for c in SV.CASES}) == len(SV.CASES)


@pytest.mark.parametrize("g,dtype,f,ld", SV.FORWARD_K3)
def test_forward_k3_cases_keep_their_tail(g, dtype, f, ld):
    st = SV.stats(g)
    v = SV.expected_variant(dtype, f, (ld, ld, SV.line_ld(f, dtype)), st.rows, st.nnz, st.n_heavy,
                            st.n_hub)
    assert v[3] > 0
    assert {(d, SV.expected_variant(d, ff, (l, l, SV.line_ld(ff, d)), *SV.stats(gg)[1:])[0])
            for gg, d, ff, l in SV.FORWARD_K3} == {("fp32", 2), ("fp32", 4), ("bf16", 2),
                                                   ("bf16", 4), ("bf16", 8)}


def test_mirror_known_points():
    """Launch shapes worked out by hand from appnp_spmm.hip launch_step, among them those of
    tests/test_gpu_parity.py::test_tail_fragments (n = 2500, no heavy rows): V shrinks there, so
    only its fp32 (101, 128) case reaches a tail, at V = 2."""
    ev = SV.expected_variant
    lat = (2500, 26_000, 0, 0)
    assert ev("bf16", 15, (16, 16, 16), *lat)[:4] == (1, 16, True, 0)
    assert ev("bf16", 70, (72, 72, 72), *lat)[:4] == (2, 64, True, 0)
    assert ev("bf16", 100, (128, 128, 128), *lat)[:4] == (2, 64, True, 0)
    assert ev("fp32", 101, (128, 128, 128), *lat)[:4] == (2, 64, True, 1)
    assert ev("fp32", 129, (132, 132), 1200, 5000, 0, 0)[:4] == (4, 64, True, 1)
    assert ev("bf16", 9, (16, 16, 16), 66_000, 600_000, 0, 0) == (8, 2, False, 1, "bandwidth")
    assert ev("bf16", 65, (72, 72, 72), 66_000, 600_000, 0, 0) == (8, 16, True, 1, "bandwidth")
    assert ev("fp32", 14, (16, 16, 16), 66_000, 1_900_000, 0, 0) == (4, 4, True, 2, "bandwidth")
    assert SV.line_ld(100, "fp32") == 100 and SV.line_ld(15, "bf16") == 16
    assert SV.line_ld(7, "fp32") == 8 and SV.line_ld(100, "bf16") % 8 == 0
    assert np.gcd(SV.line_ld(129, "fp32"), 4) == 4
