#!/usr/bin/env python3
"""Measure the forward-push PPR columns (appnp_push_columns) against the solver's columns.

Writes profiles/push_columns.json.  Per workload -- the Cora-ML fixture and arxiv-synth (169 k
nodes), 'sym', alpha = 0.1, one chunk of 128 sources -- and per eps in {1e-4, 1e-5}:

  push_ms        device time of ops.push_columns between two events (its launches and the gaps)
  kernel_ms      its launches under the library's per-launch timer (ops.kernel_times), split into
                 "push" (the round loop) and "copy" (clear, thresholds, p -> X)
  solve_ms       ppr_columns(tol=1e-6) on the same sources: the route the sparse rows had before
  rounds         of the 128 columns (max, mean); left_max = 0: every column met its bound
  edges          entries of A_hat walked per source (mean, max), from the numpy replay
                 (tests/push_ref.py) of the same sources, which must also reproduce the
                 device's columns bit for bit
  max_abs_diff   against the solver's columns, with the largest eps * sqrt(d_j) for scale

Usage: python tools/push_measure.py [--out DIR] [--reps N]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ppnp_amd  # noqa: E402
import push_ref  # noqa: E402
from ppnp_amd import ops  # noqa: E402
from ppnp_amd.ppr import ppr_columns  # noqa: E402
from ppnp_amd.synth import CONFIGS, SEEDS, uniform_graph  # noqa: E402

DEV = "cuda:0"
ALPHA, TOL, B, REPLAYED = 0.1, 1e-6, 128, 128


def wall_ms(fn, reps):
    out = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out[1:])


def measure(name, G, reps):
    n = G.n
    src = np.sort(np.random.default_rng(0).choice(n, B, replace=False))
    idx = torch.from_numpy(src).to(DEV)
    rp, col, val, dinv = (t.cpu().numpy() for t in G.csr())
    w = 1.0 / dinv
    solve = lambda: ppr_columns(G, idx, alpha=ALPHA, tol=TOL)  # noqa: E731
    exact = solve()
    solve_ms = wall_ms(solve, reps)
    rows = []
    for eps in (1e-4, 1e-5):
        push = lambda: ops.push_columns(G, idx, ALPHA, eps)  # noqa: E731
        X, rounds, left = push()
        split = {"push": [], "copy": []}
        for _ in range(reps + 1):
            t = ops.kernel_times(push, torch.device(DEV), 16)
            for kind in split:
                split[kind].append(sum(ms for k, ms in t if k == kind))
        Xr, rr, lr, edges = push_ref.push_columns(rp, col, val, src[:REPLAYED], ALPHA, eps, w)
        bits = np.array_equal(X[:, :REPLAYED].cpu().numpy().view(np.uint32), Xr.view(np.uint32))
        rounds, left = rounds.cpu().numpy(), left.cpu().numpy()
        push_ms = wall_ms(push, reps)
        rows.append({
            "workload": name, "nodes": n, "nnz_hat": G.nnz_hat, "b": B, "eps": eps,
            "push_ms": push_ms,
            "kernel_ms": {k: statistics.median(v[1:]) for k, v in split.items()},
            "launches": len(t), "solve_ms": solve_ms,
            "solve_steps": ops.solve_iterations(ALPHA, TOL),
            "push_over_solve": push_ms / solve_ms,
            "rounds_max": int(rounds.max()), "rounds_mean": float(rounds.mean()),
            "left_max": int(left.max()),
            "edges_mean": float(edges.mean()), "edges_max": int(edges.max()),
            "replayed_sources": REPLAYED, "replay_bit_identical": bool(bits)
            and bool(np.array_equal(rounds[:REPLAYED], rr)),
            "max_abs_diff_to_solver": float((X - exact).abs().max()),
            "eps_w_max": float(eps * w.max())})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    g = np.load(os.path.join(ROOT, "tests", "golden", "cora_ml.npz"), allow_pickle=False)
    n = int(g["n"])
    adj = sp.csr_matrix((g["adj_data"], g["adj_indices"], g["adj_indptr"]), shape=(n, n))
    rows = measure("cora-ml-real", ppnp_amd.Graph.from_scipy(adj, device=DEV), args.reps)
    n, medges, _ = CONFIGS["arxiv-synth"][:3]
    ip, ix = uniform_graph(n, medges, SEEDS["arxiv-synth"], device=DEV)
    rows += measure("arxiv-synth", ppnp_amd.Graph.from_csr(ip, ix, None, n, device=DEV,
                                                           features=B), args.reps)
    info = ppnp_amd._lib.load().appnp_build_info().decode()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "push_columns.json"), "w") as fh:
        json.dump({"tool": "tools/push_measure.py", "device": torch.cuda.get_device_name(0),
                   "library": info, "reps": args.reps, "alpha": ALPHA, "mode": "sym",
                   "results": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
