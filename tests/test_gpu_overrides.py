"""GPU: the launch paths of the step kernels and of the remainder pass that the default
configuration reaches only on graphs larger than any test, or only under a tuning override.

  capped grid     APPNP_MAX_BLOCKS = 1 and 7: the grid-stride loops of k_step_wide (hub rows
                  first, skipped by the regular pass) and k_step_narrow run more than one trip
  heavy blocks    graph Bh has 17 000 heavy rows, more than the 16 384 waves of a narrow
                  launch's heavy blocks: their loop runs a second trip with no override
  unrolls, hints  APPNP_UW = 4, APPNP_UN = 4, APPNP_NT = 7: kernels the sweeps of tools/ timed
  source blocks   APPNP_SB_ROWS = 1024 gives a 66 000-node graph 65 source blocks (three barrier
                  rounds of 32 on the W8 / W16 passes); with APPNP_REM_SYNC_W4 = 2 the W4 pass
                  takes the barrier loop too

The overrides are read once per process, so each configuration is one child process
(tests/override_worker.py on the product library).  tests/test_step_variants.py proves on the
host that the cases reach these paths; profiles/override_paths_hit.txt is the kernel trace.

Bars.  Every output: the fp32 bar of tests/test_gpu_parity.py (close_fp32) against the fp64
oracle, bf16 max|Z - Z_ref| <= 2e-2 max|Z_ref|; padding of the output views still NaN; run to
run bitwise equal.  A capped grid changes which wave computes a row, an unroll how many gathers
are in flight, a cache hint nothing in the arithmetic: the row's fmaf chain keeps its order, so
those children must reproduce this process's default run bit for bit, and so must the two
source-block children each other (barriers do not change arithmetic).  Against the default block
size the source-block children sum in another order: the oracle bar alone.

What the cases can and cannot see.  A hub row that the regular pass of k_step_wide fails to skip
is computed twice with the same value, which a forward step hides; only an epilogue that
accumulates (the adjoint's dH) shows it, and only when the two turns fall into different trips of
the loop -- L1's hub row is row 0, whose two turns share the first trip, so the wide adjoint on
Bsh (hub row 12 345) is the case that catches it.  The directed graph D has no heavy or hub row
in A_hat or A_hat^T: it is the transposed CSR without lists; the adjoints on Dh (six heavy rows
and a hub row in A_hat^T only) are the ones that run the t_heavy / t_hub lists.  APPNP_UN = 4 changes a kernel only in the
narrow launch of the latency regime (U = 8 at V <= 2 by default): the Md F = 7 case.

After a child ends by a signal or a time limit, every later test of the module fails at once and
starts no further process.
"""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

import override_worker as W
import step_variants as SV
from oracle import ppnp_oracle as O
from test_gpu_parity import close_fp32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 110
# appnp_tuning_overrides lists the active overrides in this order (kTuningNames)
NAME_ORDER = ["APPNP_SPLIT", "APPNP_VEC", "APPNP_WIDE", "APPNP_UW", "APPNP_UN", "APPNP_NT",
              "APPNP_MAX_BLOCKS", "APPNP_REM_SYNC_W4", "APPNP_REM_SYNC_W8", "APPNP_REM_SYNC_W16",
              "APPNP_SB_ROWS", "APPNP_REM_VF"]

CHILDREN = {
    "max-blocks-1": ("capped", {"APPNP_MAX_BLOCKS": "1"}),
    "max-blocks-7": ("capped-bh", {"APPNP_MAX_BLOCKS": "7"}),
    "uw-4": ("unroll", {"APPNP_UW": "4"}),
    "un-4": ("unroll", {"APPNP_UN": "4"}),
    "nt-7": ("unroll", {"APPNP_NT": "7"}),
    "sb-1024": ("sb", {"APPNP_SB_ROWS": str(SV.SB_ROWS)}),
    "sb-1024-sync-w4": ("sb", {"APPNP_SB_ROWS": str(SV.SB_ROWS), "APPNP_REM_SYNC_W4": "2"}),
}

_DEAD = []     # names of children that ended by a signal or a time limit
_RESULTS = {}  # child name -> its arrays, or the text of its failure


def _alive():
    """Fail at once when a child has ended by a signal or a time limit: no GPU work after it."""
    if _DEAD:
        pytest.fail(f"child {_DEAD[0]} ended by a signal or a time limit: no further GPU work")


def _child(name, tmp_path_factory):
    """The arrays child ``name`` wrote; it is started once, never again after a failure."""
    _alive()
    if name in _RESULTS:
        if isinstance(_RESULTS[name], str):
            pytest.fail(f"child {name} failed earlier:\n{_RESULTS[name]}")
        return _RESULTS[name]
    case_set, overrides = CHILDREN[name]
    out = tmp_path_factory.mktemp(name) / "out.npz"
    # the product library with nothing but the overrides asked for
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("APPNP_") and k != "PPNP_AMD_LIB"}
    env.update(overrides, APPNP_TUNING="1", PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "override_worker.py"), "--set", case_set,
           "--out", str(out)]
    t0 = time.perf_counter()
    try:
        proc = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True,
                              timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _DEAD.append(name)
        _RESULTS[name] = "time limit"
        pytest.fail(f"child {name} ran into its {CHILD_TIMEOUT} s limit")
    wall = time.perf_counter() - t0
    tail = proc.stdout[-3000:] + proc.stderr[-3000:]
    if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139):
        _DEAD.append(name)
        _RESULTS[name] = tail
        pytest.fail(f"child {name} ended with {proc.returncode}:\n{tail}")
    if proc.returncode != 0:
        _RESULTS[name] = tail
        pytest.fail(f"child {name} failed ({proc.returncode}):\n{tail}")
    with np.load(out, allow_pickle=False) as z:
        res = {k: z[k] for k in z.files}
    print(f"child {name}: {wall:.1f} s wall, {float(res['seconds']):.1f} s in main()")
    want = ";".join(f"{k}={overrides[k]}" for k in NAME_ORDER if k in overrides)
    got = str(res["overrides"])
    if got != want:  # a child that silently ran the defaults
        _RESULTS[name] = f"overrides '{got}', asked for '{want}'"
        pytest.fail(f"child {name} reports {_RESULTS[name]}")
    _RESULTS[name] = res
    return res


# ---------------------------------------------------------------------------------------
# this process: the default run and the fp64 oracle
# ---------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def defaults():
    """Every step-kernel case in this process, with no override active."""
    _alive()
    assert not os.environ.get("APPNP_TUNING"), "run the suite without APPNP_TUNING"
    assert W.overrides() == b""
    res = W.run_set("capped-bh")
    res.update(W.run_set("unroll"))
    return res


def values(raw, f, dtype):
    """The [:, :f] values of a raw output buffer as fp64, after asserting that its padding is
    still NaN (never written) and the values finite (no padding or stale memory read)."""
    x = raw if dtype == "fp32" else (raw.astype(np.uint32) << 16).view(np.float32)
    assert np.isnan(x[:, f:]).all(), "output padding was written"
    out = x[:, :f].astype(np.float64)
    assert np.isfinite(out).all(), "padding (NaN) or stale memory reached the result"
    return out


_ORACLE = {}


def oracle(c):
    cid = SV.ocase_id(c)
    if cid not in _ORACLE:
        x = W.ocase_input(c).astype(np.float64)
        if isinstance(c, SV.SpmmCase):
            A = SV.spmm_matrix().astype(np.float64)
            if c.p_drop > 0:  # the key of entry (i, j) is (j, i): the mask of A^T's entry
                assert c.transposed_key
                A = O.masked_operator(A.T.tocsr(), 0, c.p_drop, SV.O_SEED).T.tocsr()
            _ORACLE[cid] = A @ x
        else:
            fn = O.appnp_propagate if c.op == "fwd" else O.appnp_backward
            _ORACLE[cid] = fn(SV.a_hat(c.graph, c.mode), x, c.K, SV.O_ALPHA, c.p_drop, SV.O_SEED)
    return _ORACLE[cid]


def check_oracle(c, raw):
    dtype = "fp32" if isinstance(c, SV.SpmmCase) else c.dtype
    got, ref = values(raw, c.f, dtype), oracle(c)
    err = np.abs(got - ref).max()
    print(f"{SV.ocase_id(c)}: max err {err:.3e}, max|ref| {np.abs(ref).max():.3e}")
    if dtype == "fp32":
        close_fp32(got, ref)
    else:
        assert err <= 2e-2 * np.abs(ref).max(), SV.ocase_id(c)


def check_set(cases, res, base=None):
    """Every case of ``res``: the oracle bar, run to run bitwise equal, and (``base``: the
    default run) bitwise equal to it."""
    for c in cases:
        cid = SV.ocase_id(c)
        check_oracle(c, res[cid])
        assert bool(res["same__" + cid]), f"{cid}: two runs differ"
        if base is not None:
            a, b = W.bits(res[cid]), W.bits(base[cid])
            assert a.shape == b.shape
            diff = int((a != b).sum())
            assert diff == 0, f"{cid}: {diff} of {a.size} elements differ from the default run"


def test_parent_runs_the_defaults(defaults):
    _alive()
    assert W.overrides() == b""
    check_set(SV.OVERRIDE_CAPPED + SV.OVERRIDE_UNROLL, defaults)


def test_heavy_block_loop(defaults):
    """Bh in this process: 17 000 heavy rows on 4096 x 4 waves."""
    _alive()
    for c in SV.OVERRIDE_BH:
        v = SV.ocase_variant(c)
        st = SV.ocase_launch(c)[2]
        assert not v[2] and SV.expected_grid(v, st.rows, st.n_hub, st.n_heavy, f=c.f)[1] == 4096
        assert st.n_heavy > 4096 * SV.K_WAVES_PER_BLOCK
    check_set(SV.OVERRIDE_BH, defaults)


@pytest.mark.parametrize("name", ["max-blocks-1", "max-blocks-7"])
def test_capped_grid(defaults, tmp_path_factory, name):
    res = _child(name, tmp_path_factory)
    check_set(SV.OVERRIDE_SETS[CHILDREN[name][0]], res, defaults)


@pytest.mark.parametrize("name", ["uw-4", "un-4", "nt-7"])
def test_unrolls_and_cache_policy(defaults, tmp_path_factory, name):
    res = _child(name, tmp_path_factory)
    check_set(SV.OVERRIDE_UNROLL, res, defaults)


# ---------------------------------------------------------------------------------------
# the remainder pass over 65 source blocks
# ---------------------------------------------------------------------------------------


def sb_oracle(gname, weighted, modes, c):
    key = ("sb", gname, c)
    if key not in _ORACLE:
        ah = O.calc_a_hat(SV.sb_adjacency(weighted), modes[c.width])
        fn = O.appnp_propagate if c.op == "fwd" else O.appnp_backward
        _ORACLE[key] = fn(ah, W.sb_input(gname, c).astype(np.float64), SV.SB_K, SV.O_ALPHA,
                          c.p_drop, SV.O_SEED)
    return _ORACLE[key]


def sb_ids():
    return [(g, c) for g, _, _ in SV.SB_GRAPHS for c in SV.sb_cases_of(g)]


@pytest.mark.parametrize("name", ["sb-1024", "sb-1024-sync-w4"])
def test_many_source_blocks(tmp_path_factory, name):
    """The child asserts 65 source blocks and K remainder launches per call; here every output
    against the fp64 oracle."""
    res = _child(name, tmp_path_factory)
    for gname, weighted, modes in SV.SB_GRAPHS:
        for c in SV.sb_cases_of(gname):
            cid = SV.sb_case_id(gname, c)
            got = values(res[cid], c.f, "fp32")
            ref = sb_oracle(gname, weighted, modes, c)
            print(f"{cid}: max err {np.abs(got - ref).max():.3e}, max|ref| {np.abs(ref).max():.3e}")
            close_fp32(got, ref)
            assert bool(res["same__" + cid]), f"{cid}: two runs differ"


def test_barriers_do_not_change_the_sums(tmp_path_factory):
    a = _child("sb-1024", tmp_path_factory)
    b = _child("sb-1024-sync-w4", tmp_path_factory)
    for gname, c in sb_ids():
        cid = SV.sb_case_id(gname, c)
        diff = int((W.bits(a[cid]) != W.bits(b[cid])).sum())
        assert diff == 0, f"{cid}: {diff} elements differ between the two barrier settings"
