#!/usr/bin/env python
"""Child process of tests/test_gpu_overrides.py: the step kernels and the remainder pass under a
tuning override, on the product library.

    APPNP_TUNING=1 APPNP_MAX_BLOCKS=7 python tests/override_worker.py --set capped-bh --out o.npz

The overrides (include/ppnp_amd.h appnp_tuning_overrides) are read once per process, so every
configuration is a process of its own; the parent sets the environment.  ``--set`` names a table
of tests/step_variants.py (OVERRIDE_SETS) or ``sb`` (SB_CASES, the remainder pass with 65 source
blocks, which needs APPNP_SB_ROWS=1024).  Every case runs twice.  out.npz holds, per case id, the
whole output buffer of the first run (fp32 values, or bf16 bit patterns as uint16; padded views
start NaN-filled, so the parent can see what was written), ``same__<id>`` (the second run was
bitwise the same), ``overrides`` (the string the library reports) and ``seconds``.

The parent imports this module too and calls ``run_set`` in its own process, without overrides,
for the outputs that a capped grid, another unroll or a cache hint must reproduce bit for bit.
``--trace-plan FILE`` writes the kernel and grid that tests/step_variants.py predicts for every
step launch, in launch order (tools/override_paths.py compares a kernel trace with it).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import step_variants as SV  # noqa: E402

_GRAPHS = {}


def overrides():
    from ppnp_amd import _lib

    return _lib.load().appnp_tuning_overrides()


def ocase_input(c):
    """The case's H (forward) or dZ (adjoint) as fp32 numpy; bf16 cases hold bf16 values."""
    if isinstance(c, SV.SpmmCase):
        return SV.randn((SV.SPMM_COLS, c.f), SV.ocase_seed(c), "fp32")
    n = SV.adjacency(c.graph).shape[0]
    return SV.randn((n, c.f), SV.ocase_seed(c), c.dtype)


def raw(buf):
    """A device buffer as numpy: fp32 values, or the bit patterns of bf16 ones."""
    import torch

    if buf.dtype == torch.bfloat16:
        return buf.view(torch.int16).cpu().numpy().view(np.uint16)
    return buf.cpu().numpy()


def bits(a):
    return a if a.dtype == np.uint16 else a.view(np.uint32)


def _graph(c):
    import ppnp_amd as pa

    key = (c.graph, c.mode, c.transpose)
    if key not in _GRAPHS:
        G = pa.Graph.from_scipy(SV.adjacency(c.graph), mode=c.mode, device=SV.DEV,
                                transpose=c.transpose)
        st = SV.ostats(c.graph, c.mode)
        assert (G.n, G.rows, G.nnz_hat) == (st.n, st.rows, st.nnz), (key, G)
        assert G.source_block_bytes() == 0  # whole rows: the step kernels take every column
        _GRAPHS[key] = G
    return _GRAPHS[key]


def _spmm_operands():
    import torch

    if "spmm" not in _GRAPHS:
        A = SV.spmm_matrix()
        _GRAPHS["spmm"] = tuple(torch.from_numpy(x).to(SV.DEV)
                                for x in (A.indptr, A.indices, A.data))
    return _GRAPHS["spmm"]


def run_ocase(c):
    """One run of the case; returns the raw output buffer."""
    import torch

    import ppnp_amd as pa

    x = ocase_input(c)
    if isinstance(c, SV.SpmmCase):
        from ppnp_amd.sparse import spmm

        ip, ix, dv = _spmm_operands()
        out = torch.full((SV.SPMM_ROWS, c.f), float("nan"), device=SV.DEV)
        spmm(ip, ix, dv, SV.SPMM_ROWS, SV.SPMM_COLS, torch.from_numpy(x).to(SV.DEV),
             p_drop=c.p_drop, seed=SV.O_SEED, transposed_key=c.transposed_key, out=out)
        return raw(out)
    G = _graph(c)
    _, X = SV.operand(x, c.ld, c.dtype)
    buf, out = SV.blank(G.n, c.f, c.ld, c.dtype)
    if c.op == "fwd":
        pa.propagate_forward(G, X, c.K, SV.O_ALPHA, p_drop=c.p_drop, seed=SV.O_SEED, out=out)
    else:
        SV.propagate_backward_views(G, X, out, c.K, SV.O_ALPHA, c.p_drop, SV.O_SEED)
    return raw(buf)


def run_set(name):
    """{case id: raw output, "same__<id>": second run bitwise equal} over OVERRIDE_SETS[name]."""
    res = {}
    for c in SV.OVERRIDE_SETS[name]:
        a, b = run_ocase(c), run_ocase(c)
        res[SV.ocase_id(c)] = a
        res["same__" + SV.ocase_id(c)] = np.array(np.array_equal(bits(a), bits(b)))
    return res


# ---- the remainder pass with many source blocks -------------------------------------------


def sb_input(gname, c):
    return SV.randn((SV.SB_N, c.f), c.f * 17 + c.width + (3 if c.op == "bwd" else 0)
                    + (1000 if gname == "weighted" else 0), "fp32")


def _source_blocks(G, weighted, mode):
    """nb of the graph's source-blocked copy.  The ABI does not report it, so it is recovered
    from the byte count of appnp_graph_source_blocks (appnp_capi.hip), whose formula this
    mirrors: rb_total entries (8 B with values, 4 without) + rb_total / 16 * lpe bytes of chunk
    table + (passes * nb * slots + 1) int32 segment offsets + 4 n bytes per fp32 scale vector of a
    value-free copy (dl; dr too for 'sym'), slots = CUs * kRemWaves (16).  If that accounting
    changes, the assertion below fails and names this formula, not nb."""
    import torch

    lay = G.source_block_layout()
    assert lay is not None and lay["value_free"] == (not weighted), lay
    lpe = lay["width"] // 4
    total = lay["entries"]
    scales = 0 if weighted else (2 if mode == "sym" else 1) * G.n * 4
    cells4 = G.source_block_bytes() - total * (8 if weighted else 4) - total // 16 * lpe - scales
    slots = torch.cuda.get_device_properties(G.device).multi_processor_count * 16  # kRemWaves
    nb, left = divmod(cells4 // 4 - 1, lay["row_passes"] * slots)
    assert cells4 % 4 == 0 and left == 0, (
        "the byte formula of appnp_graph_source_blocks mirrored in _source_blocks no longer "
        f"holds: {cells4} offset bytes, layout {lay}, {slots} slots")
    return nb


def run_sb():
    """SB_CASES on the unit and the weighted graph, each twice; asserts on the way that every
    case took the remainder pass (SB_K launches per call) over SB_NB source blocks."""
    import ppnp_amd as pa

    res = {}
    for gname, weighted, modes in SV.SB_GRAPHS:
        adj = SV.sb_adjacency(weighted)
        for w, feats in SV.SB_FEATURES.items():
            mode = modes[w]
            G = pa.Graph.from_scipy(adj, mode=mode, device=SV.DEV, features=feats)
            assert G.source_block_layout()["width"] == w
            nb = _source_blocks(G, weighted, mode)
            assert nb == SV.SB_NB, f"{gname} W{w}: {nb} source blocks, not {SV.SB_NB}"
            for c in SV.sb_cases_of(gname):
                if c.width != w:
                    continue
                r = c.f % 32 if c.f > 32 else c.f
                assert G.remainder_cols(c.f) == r and G.split_point(c.f) == c.f - r
                ld = SV.pad4(c.f)
                _, X = SV.operand(sb_input(gname, c), ld, "fp32")
                runs = []
                for _ in range(2):
                    buf, out = SV.blank(G.n, c.f, ld, "fp32")
                    before = G.source_block_layout()["launches"]
                    if c.op == "fwd":
                        pa.propagate_forward(G, X, SV.SB_K, SV.O_ALPHA, p_drop=c.p_drop,
                                             seed=SV.O_SEED, out=out)
                    else:
                        SV.propagate_backward_views(G, X, out, SV.SB_K, SV.O_ALPHA, c.p_drop,
                                                    SV.O_SEED)
                    took = G.source_block_layout()["launches"] - before
                    assert took == SV.SB_K, f"{SV.sb_case_id(gname, c)}: {took} remainder launches"
                    runs.append(raw(buf))
                cid = SV.sb_case_id(gname, c)
                res[cid] = runs[0]
                res["same__" + cid] = np.array(np.array_equal(bits(runs[0]), bits(runs[1])))
            G.close()
    return res


# ---- the launches tests/step_variants.py predicts, in order --------------------------------


def trace_plan(name, env):
    """[{case, kernel, grid}] per step launch of the set under the overrides in ``env``."""
    mb = int(env.get("APPNP_MAX_BLOCKS", SV.K_MAX_BLOCKS))
    uw = int(env["APPNP_UW"]) if "APPNP_UW" in env else None
    un = int(env["APPNP_UN"]) if "APPNP_UN" in env else None
    plan = []
    if name == "sb":  # k_rem_persist<EPI, U, VF, LPE> on one workgroup per CU (grid unknown here)
        for gname, weighted, modes in SV.SB_GRAPHS:
            for w in SV.SB_FEATURES:
                for c in SV.sb_cases_of(gname):
                    if c.width != w:
                        continue
                    lpe = w // 4
                    kernel = (f"k_rem_persist<{0 if c.op == 'fwd' else 1}, {4 if lpe == 4 else 2}, "
                              f"{'false' if weighted else 'true'}, {lpe}>")
                    plan += [{"case": SV.sb_case_id(gname, c), "kernel": kernel,
                              "grid": [None, 1]}] * (2 * SV.SB_K)
        return plan
    for c in SV.OVERRIDE_SETS[name]:
        kernel, grid = SV.ocase_prediction(c, mb, uw, un)
        launches = 1 if isinstance(c, SV.SpmmCase) else c.K
        for _ in range(2 * launches):  # every case runs twice
            plan.append({"case": SV.ocase_id(c), "kernel": kernel, "grid": list(grid)})
    return plan


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--set", required=True, choices=sorted(SV.OVERRIDE_SETS) + ["sb"])
    p.add_argument("--out", required=True)
    p.add_argument("--trace-plan")
    a = p.parse_args()

    import torch

    from ppnp_amd import _lib

    # the product library, whatever the caller's environment names
    info = _lib.load().appnp_build_info().decode()
    assert os.path.samefile(_lib.LIB_PATH, os.path.join(os.path.dirname(_lib.__file__),
                                                        "libppnp_amd.so")), _lib.LIB_PATH
    assert "testing=1" not in info, info
    t0 = time.perf_counter()
    env = {k: v for k, v in os.environ.items() if k.startswith("APPNP_")}
    if a.trace_plan:
        with open(a.trace_plan, "w") as fh:
            json.dump(trace_plan(a.set, env if env.get("APPNP_TUNING") == "1" else {}), fh)
    res = run_sb() if a.set == "sb" else run_set(a.set)
    torch.cuda.synchronize()
    res["overrides"] = np.array(overrides().decode())
    res["seconds"] = np.array(time.perf_counter() - t0)
    np.savez(a.out, **res)
    print(f"[override_worker] {a.set}: {len(res) // 2 - 1} cases, overrides "
          f"'{overrides().decode()}', {float(res['seconds']):.1f} s", flush=True)


if __name__ == "__main__":
    main()
