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


# ---------------------------------------------------------------------------------------
# the override cases of tests/test_gpu_overrides.py reach the paths they are there for
# ---------------------------------------------------------------------------------------


def _is_step(c):
    return not isinstance(c, SV.SpmmCase)


def test_graph_bh_has_more_heavy_rows_than_heavy_waves():
    st = SV.stats("Bh")
    assert st.n == SV.BH_N == 100_000
    assert st.n_heavy == 17_000 > SV.K_HEAVY_BLOCKS * SV.K_WAVES_PER_BLOCK == 16384
    assert st.n_hub == 0 and st.nnz < SV.K_WIDE_AVG_ROW * st.n
    adj = SV.adjacency("Bh")
    assert (adj != adj.T).nnz == 0 and adj.diagonal().sum() == 0 and set(adj.data) == {1.0}
    lens = np.diff(SV.a_hat("Bh").indptr)
    assert (lens[:SV.BH_HEAVY] == 34).all() and 34 > SV.K_HEAVY_ROW
    assert set(lens[SV.BH_HEAVY:]) == {7, 8}  # the light rows: at most kHeavyRow entries
    assert abs(st.nnz / st.n - 12.2) < 0.05
    for c in SV.OVERRIDE_BH:
        v = SV.ocase_variant(c)
        s = SV.ocase_launch(c)[2]
        assert not v[2] and v[4] == "bandwidth", SV.ocase_id(c)  # a narrow launch
        light, heavy, _ = SV.expected_grid(v, s.rows, s.n_hub, s.n_heavy, f=c.f)
        assert heavy == 4096 and light == SV.uncapped_blocks(v, s.rows, s.n_hub)
        # the heavy loop's stride is heavy * 4 waves: rows past it take a second trip
        assert s.n_heavy > heavy * SV.K_WAVES_PER_BLOCK
    assert {(c.dtype, c.op) for c in SV.OVERRIDE_BH} == {("fp32", "fwd"), ("fp32", "bwd"),
                                                         ("bf16", "fwd")}


@pytest.mark.parametrize("cap", [1, 7])
def test_capped_cases_take_a_second_trip(cap):
    cases = SV.OVERRIDE_CAPPED + (SV.OVERRIDE_BH if cap == 7 else [])
    for c in cases:
        cid = SV.ocase_id(c)
        v = SV.ocase_variant(c)
        s = SV.ocase_launch(c)[2]
        uncapped = SV.uncapped_blocks(v, s.rows, s.n_hub)
        light, heavy, _ = SV.expected_grid(v, s.rows, s.n_hub, s.n_heavy, cap, f=c.f)
        assert uncapped > cap and light == cap, cid            # the cap binds
        total = s.rows + (s.n_hub if v[2] else 0)
        per_trip = cap * SV.rows_per_block(v)
        assert total / per_trip > 1, cid                       # the loop iterates
        if cap == 7:
            assert total % per_trip != 0, cid                  # and its last trip is ragged
            if not (_is_step(c) and c.graph == "L1"):
                assert uncapped % 7 != 0, cid
        assert heavy == (0 if v[2] else min((s.n_heavy + 3) // 4, 4096)), cid
    # L1's 4000 rows and one hub row make 1001 = 7 * 143 blocks of four waves: the uncapped grid
    # IS a multiple of 7 there, but the 4001 virtual rows are no multiple of the 28 waves, so the
    # last trip still leaves waves without a row (asserted above for every case of cap 7)
    l1 = [c for c in SV.OVERRIDE_CAPPED if _is_step(c) and c.graph == "L1"]
    assert l1 and all(SV.uncapped_blocks(SV.ocase_variant(c), 4000, SV.stats("L1").n_hub) == 1001
                      for c in l1)
    step = [c for c in SV.OVERRIDE_CAPPED if _is_step(c)]
    # wide launches on L1 and Bsh dispatch hub rows first; the narrow Bsh ones append heavy blocks
    wide_hub = [c for c in step if c.graph in ("L1", "Bsh") and SV.ocase_variant(c)[2]]
    assert {c.graph for c in wide_hub} == {"L1", "Bsh"}
    assert all(SV.ocase_launch(c)[2].n_hub >= 1 for c in wide_hub)
    # and one of them is an adjoint whose hub row takes its two turns in different trips
    hub_row = int(np.flatnonzero(np.diff(SV.a_hat("Bsh").indptr) > SV.K_HUB_ROW)[0])
    assert any(c.graph == "Bsh" and c.op == "bwd" for c in wide_hub)
    assert hub_row + 1 >= 2 * 7 * SV.K_WAVES_PER_BLOCK
    narrow_bsh = [c for c in step if c.graph == "Bsh" and not SV.ocase_variant(c)[2]]
    assert len(narrow_bsh) == 3 and all(SV.ocase_launch(c)[2].n_heavy > 0 for c in narrow_bsh)
    assert not SV.ocase_variant(next(c for c in step if c.graph == "Bs"))[2]
    d = [c for c in step if c.graph == "D"]
    assert {(c.op, c.mode, c.transpose) for c in d} == {("fwd", "rw", True), ("bwd", "rw", True)}
    # D is the transposed CSR without lists (no heavy or hub row either way); the lists of
    # A_hat^T are reached by Dh's adjoints: t_heavy in the heavy blocks of the narrow launch,
    # t_hub first in the wide one, its hub row taking its two turns in different trips
    for t in (False, True):
        assert (SV.ostats("D", "rw", t).n_heavy, SV.ostats("D", "rw", t).n_hub) == (0, 0)
    fw, tr = SV.ostats("Dh", "rw"), SV.ostats("Dh", "rw", True)
    assert (fw.n_heavy, fw.n_hub) == (0, 0) and tr.n_heavy == 6 and tr.n_hub == 1
    assert tr.n > SV.K_LATENCY_ROWS and tr.nnz < SV.K_WIDE_AVG_ROW * tr.n
    adj = SV.adjacency("Dh")
    assert (adj != adj.T).nnz > 0 and adj.diagonal().sum() == 0
    t_lens = np.diff(SV.a_hat("Dh", "rw").T.tocsr().indptr)
    assert int(np.flatnonzero(t_lens > SV.K_HUB_ROW)[0]) + 1 >= 2 * 7 * SV.K_WAVES_PER_BLOCK
    dh = [c for c in step if c.graph == "Dh"]
    assert all((c.op, c.mode, c.transpose) == ("bwd", "rw", True) for c in dh)
    assert sorted(SV.ocase_variant(c)[2] for c in dh) == [False, True]
    for c in dh:
        assert SV.ocase_launch(c)[2] == tr
        heavy = SV.expected_grid(SV.ocase_variant(c), tr.rows, tr.n_hub, tr.n_heavy, 7, f=c.f)[1]
        assert heavy == (0 if SV.ocase_variant(c)[2] else 2)
    assert {c.f for c in SV.OVERRIDE_CAPPED if not _is_step(c)} == {130, 7}
    assert sum(1 for c in SV.OVERRIDE_CAPPED if not _is_step(c) and c.transposed_key) == 1


def test_unroll_overrides_select_other_instantiations():
    """APPNP_UW = 4 names an instantiation no default launch runs, for every wide case; APPNP_UN
    = 4 changes the narrow kernel of the latency regime (U = 8 at V <= 2 by default)."""
    wide = [c for c in SV.OVERRIDE_UNROLL if SV.ocase_variant(c)[2]]
    narrow = [c for c in SV.OVERRIDE_UNROLL if not SV.ocase_variant(c)[2]]
    assert {c.graph for c in wide} == {"L1", "Bl", "Md"} and {c.graph for c in narrow} == {"Bs", "Md"}
    default_names = {SV.ocase_prediction(c)[0] for c in SV.OVERRIDE_UNROLL}
    for c in wide:
        uw4 = SV.ocase_prediction(c, uw=4)[0]
        assert uw4 != SV.ocase_prediction(c)[0] and ", 4, " in uw4, SV.ocase_id(c)
        assert uw4 not in default_names
        assert SV.ocase_prediction(c, un=4) == SV.ocase_prediction(c)
    assert {SV.ocase_prediction(c)[0].split(", ")[4] for c in wide} == {"8", "2", "1"}
    changed = [c for c in narrow if SV.ocase_prediction(c, un=4)[0] != SV.ocase_prediction(c)[0]]
    assert [(c.graph, c.f) for c in changed] == [("Md", 7)]
    assert {(c.graph, c.op) for c in SV.OVERRIDE_UNROLL if c.op == "bwd"} == {("L1", "bwd")}


def test_expected_grid_known_points():
    """launch_step's grid worked out by hand."""
    wide = (4, 32, True, 0, "bandwidth")
    narrow = (2, 4, False, 1, "bandwidth")
    assert SV.expected_grid(wide, 66_000, 1, 6, f=66) == (16501, 0, 1)     # hub row counted
    assert SV.expected_grid(narrow, 66_000, 1, 6, f=7) == (1032, 2, 1)     # hub dropped, 6 heavy
    assert SV.expected_grid(narrow, 66_000, 1, 6, 7, f=7) == (7, 2, 1)
    assert SV.expected_grid(narrow, 100_000, 0, 17_000, f=7)[1] == 4096
    assert SV.expected_grid(wide, 17_000_000, 0, 0, f=66)[0] == 1 << 22           # the shipped cap
    assert SV.expected_grid((2, 64, True, 0, "latency"), 900, 0, 0, f=130) == (225, 0, 2)
    assert SV.expected_grid(wide, 66_000, 1, 6, 1 << 30, f=66)[0] == 16501       # never above 2^22


def test_source_block_cases():
    """The remainder-pass cases: 65 blocks of 1024 rows, three barrier rounds of 32, and widths
    that split where the child asserts they do."""
    assert (SV.SB_N + SV.SB_ROWS - 1) // SV.SB_ROWS == SV.SB_NB == 65
    assert SV.SB_N > SV.K_LATENCY_ROWS
    assert [b for b in range(0, SV.SB_NB, 32)] == [0, 32, 64]  # the last round: one block
    from ppnp_amd.graph import remainder_width

    for w, f in SV.SB_FEATURES.items():
        assert remainder_width(SV.SB_N, f) == w
    assert {(c.width, c.f) for c in SV.SB_CASES if c.op == "fwd" and not c.p_drop} == {
        (4, 100), (4, 36), (4, 33), (4, 3), (8, 40), (8, 37), (8, 5), (16, 13)}
    assert {(c.width, c.f) for c in SV.SB_CASES if c.p_drop} == {(4, 36), (8, 40)}
    assert {(c.width, c.f) for c in SV.SB_CASES if c.op == "bwd"} == {(4, 100), (8, 40), (16, 13)}
    adj, wgt = SV.sb_adjacency(False), SV.sb_adjacency(True)
    assert set(adj.data) == {1.0} and set(wgt.data) == {0.5, 1.0, 2.0}
    assert (wgt != wgt.T).nnz == 0 and (adj != adj.T).nnz == 0
    assert np.diff(adj.indptr).max() >= SV.SB_HUB > SV.K_HUB_ROW
