#!/usr/bin/env python3
"""Measure the exact PPNP solver (appnp_solve) against the plain series on one GPU.

Writes the two records of profiles/README.md:

  solve_step_cost.json     per-launch time (ops.kernel_times, the library's own event pairs) of
                           a Chebyshev step beside the whole-row forward step of
                           propagate_forward in the same build, and their ratio
  solve_time_to_tol.json   device time of solve(tol=1e-6) against propagate_forward with
                           K = 131 (the plain count for the same tolerance at alpha = 0.1),
                           with each one's measured error against an fp64 reference

on arxiv-synth (169 k nodes, F = 128; reference: the fp64 replay of the recurrence on a
16-column factor of H, see below) and on the Cora-ML fixture (F = 7; reference: pprH_a0.1).

Usage: python tools/solve_measure.py [--out DIR] [--reps N]
"""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ppnp_amd  # noqa: E402
from ppnp_amd import ops  # noqa: E402
from ppnp_amd.synth import CONFIGS, SEEDS, uniform_graph  # noqa: E402

DEV = "cuda:0"
ALPHA, TOL, PLAIN_K = 0.1, 1e-6, 131


def replay(a_hat, H, alpha, iters):
    prev, z = None, H
    for w in ops.solve_weights(alpha, iters):
        t = (1.0 - alpha) * (a_hat @ z) + alpha * H
        prev, z = z, (t if prev is None else w * t + (1.0 - w) * prev)
    return z


def host_a_hat(G):
    rp, col, val, _ = G.csr()
    return sp.csr_matrix((val.cpu().numpy().astype(np.float64), col.cpu().numpy(),
                          rp.cpu().numpy()), shape=(G.n, G.n))


def step_times(fn, reps):
    """Median over `reps` calls of (mean ms per "step" launch, sum of the call's launches)."""
    per, total = [], []
    for _ in range(reps + 1):
        t = [ms for kind, ms in ops.kernel_times(fn, torch.device(DEV), 4096) if kind == "step"]
        per.append(sum(t) / len(t))
        total.append(sum(t))
    return statistics.median(per[1:]), statistics.median(total[1:]), len(t)


def wall_ms(fn, reps):
    """Median device time of the whole call between two events (launch gaps included)."""
    out = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out[1:])


def measure(name, G, H, ref, reps):
    m = ops.solve_iterations(ALPHA, TOL)
    n, f = H.shape
    Z = torch.empty_like(H)
    solve = lambda: ops.solve_forward(G, H, m, ALPHA, out=Z)  # noqa: E731
    plain = lambda: ops.propagate_forward(G, H, PLAIN_K, ALPHA, out=Z)  # noqa: E731
    scale = float(np.abs(ref).max())
    solve()
    err_s = float(np.abs(Z.double().cpu().numpy() - ref).max()) / scale
    plain()
    err_p = float(np.abs(Z.double().cpu().numpy() - ref).max()) / scale
    # the first step of a solve is the plain forward step; the Chebyshev steps are the rest
    cheb = []
    for _ in range(reps + 1):
        t = [ms for kind, ms in ops.kernel_times(solve, torch.device(DEV), 4096)
             if kind == "step"]
        cheb.append(sum(t[1:]) / (len(t) - 1))
    cheb_ms = statistics.median(cheb[1:])
    fwd_ms, plain_sum, plain_n = step_times(plain, reps)
    _, solve_sum, solve_n = step_times(solve, reps)
    assert solve_n == m and plain_n == PLAIN_K
    cost = {"workload": name, "nodes": n, "F": f, "nnz_a_hat": G.nnz_hat,
            "forward_step_ms": fwd_ms, "solver_step_ms": cheb_ms, "ratio": cheb_ms / fwd_ms,
            "extra_read_bytes_per_step": n * f * 4}
    ttt = {"workload": name, "nodes": n, "F": f, "alpha": ALPHA, "tol": TOL,
           "solve": {"launches": m, "kernel_ms": solve_sum, "call_ms": wall_ms(solve, reps),
                     "err_over_max_ref": err_s},
           "plain": {"launches": PLAIN_K, "kernel_ms": plain_sum,
                     "call_ms": wall_ms(plain, reps), "err_over_max_ref": err_p}}
    ttt["speedup_kernel"] = plain_sum / solve_sum
    ttt["speedup_call"] = ttt["plain"]["call_ms"] / ttt["solve"]["call_ms"]
    ttt["speedup_launch_count"] = PLAIN_K / m
    return cost, ttt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    costs, ttts = [], []

    g = {}
    for part in ("", "_ppnp"):  # the fixture's arrays are kept in parts below 1 MiB
        g.update(np.load(os.path.join(ROOT, "tests", "golden", f"cora_ml{part}.npz"),
                         allow_pickle=False))
    n = int(g["n"])
    adj = sp.csr_matrix((g["adj_data"], g["adj_indices"], g["adj_indptr"]), shape=(n, n))
    G = ppnp_amd.Graph.from_scipy(adj, device=DEV)
    c, t = measure("cora-ml-real", G, torch.from_numpy(g["H"]).to(DEV), g["pprH_a0.1"], args.reps)
    t["reference"] = "tests/golden pprH_a0.1 (compute_ppr(adj, 0.1) @ H, fp64)"
    costs.append(c), ttts.append(t)

    n, medges, f = CONFIGS["arxiv-synth"][:3]
    ip, ix = uniform_graph(n, medges, SEEDS["arxiv-synth"], device=DEV)
    G = ppnp_amd.Graph.from_csr(ip, ix, None, n, device=DEV, features=f)
    # H = B R (B [n, 16], R [16, F]): the solve is linear and column-separable, so the fp64
    # converged reference Pi H = (Pi B) R costs a replay on 16 columns; 80 steps of it are
    # converged to 2 sigma^80 = 1e-16.  fl32(B R) differs from B R by 2^-24 per element
    # (about 1e-7 of max|ref|)
    rng = np.random.default_rng(0)
    B, R = rng.standard_normal((n, 16)), rng.standard_normal((16, f)) / 4
    ref = replay(host_a_hat(G), B, ALPHA, 80) @ R
    c, t = measure("arxiv-synth", G, torch.from_numpy((B @ R).astype(np.float32)).to(DEV), ref,
                   args.reps)
    t["reference"] = "fp64 scipy replay of the recurrence, 80 steps (converged to 1e-16), H = B R"
    costs.append(c), ttts.append(t)

    info = ppnp_amd._lib.load().appnp_build_info().decode()
    os.makedirs(args.out, exist_ok=True)
    for fname, rows in (("solve_step_cost.json", costs), ("solve_time_to_tol.json", ttts)):
        with open(os.path.join(args.out, fname), "w") as fh:
            json.dump({"tool": "tools/solve_measure.py", "device": torch.cuda.get_device_name(0),
                       "library": info, "reps": args.reps, "results": rows}, fh, indent=1)
            fh.write("\n")
        print(fname, json.dumps(rows))


if __name__ == "__main__":
    main()
