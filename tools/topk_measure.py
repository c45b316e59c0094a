#!/usr/bin/env python3
"""Measure the column top-k selection (appnp_topk_columns) against the torch route it replaces.

Writes profiles/topk_select.json.  Per workload -- the Cora-ML fixture x 128 sources and
arxiv-synth (169 k nodes) x 128 sources, k = 128, on the solver's PPR columns (tol = 1e-6):

  chain_ms       device time of ops.topk_columns between two events (its launches and the gaps)
  kernel_ms      the sum of its launches under the library's per-launch timer (ops.kernel_times)
  torch_ms       cols.t().contiguous() + topk + a sort of the indices (+ a gather of the
                 values), on the same tensor -- what ppr_rows(topk=) amounts to when the result
                 has to be a canonical CSR
  read_GBps      the chain's bytes read from X (6 passes of n * b * 4) over kernel_ms
  solve_ms       the 32-step solve that produced the columns, for scale

Usage: python tools/topk_measure.py [--out DIR] [--reps N]
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
from ppnp_amd.ppr import ppr_columns  # noqa: E402
from ppnp_amd.synth import CONFIGS, SEEDS, uniform_graph  # noqa: E402

DEV = "cuda:0"
ALPHA, TOL, B, K_SEL, PASSES = 0.1, 1e-6, 128, 128, 6


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


def torch_route(cols, k):
    rows = cols.t().contiguous()
    val, idx = rows.topk(k, dim=1)
    idx, order = idx.sort(dim=1)
    return idx, val.gather(1, order)


def measure(name, G, reps):
    n = G.n
    idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(n, B, replace=False))).to(DEV)
    cols = ppr_columns(G, idx, alpha=ALPHA, tol=TOL)
    chain = lambda: ops.topk_columns(cols, K_SEL)  # noqa: E731
    i0, v0 = chain()
    i1, v1 = torch_route(cols, K_SEL)
    # the two routes agree wherever the k-th value is not tied (torch breaks ties its own way)
    agree = float((i0.long() == i1).float().mean())
    kernel = []
    for _ in range(reps + 1):
        t = ops.kernel_times(chain, torch.device(DEV), 64)
        kernel.append(sum(ms for _, ms in t))
    kernel_ms = statistics.median(kernel[1:])
    m = ops.solve_iterations(ALPHA, TOL)
    E = torch.zeros(n, B, device=DEV)
    E[idx, torch.arange(B, device=DEV)] = 1.0
    Z = torch.empty_like(E)
    return {"workload": name, "nodes": n, "b": B, "k": K_SEL, "launches": len(t),
            "chain_ms": wall_ms(chain, reps), "kernel_ms": kernel_ms,
            "torch_ms": wall_ms(lambda: torch_route(cols, K_SEL), reps),
            "read_bytes": PASSES * n * B * 4,
            "read_GBps": PASSES * n * B * 4 / (kernel_ms * 1e-3) / 1e9,
            "solve_ms": wall_ms(lambda: ops.solve_forward(G, E, m, ALPHA, out=Z), reps),
            "solve_steps": m, "index_agreement_with_torch": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    rows = []
    g = np.load(os.path.join(ROOT, "tests", "golden", "cora_ml.npz"), allow_pickle=False)
    n = int(g["n"])
    adj = sp.csr_matrix((g["adj_data"], g["adj_indices"], g["adj_indptr"]), shape=(n, n))
    rows.append(measure("cora-ml-real", ppnp_amd.Graph.from_scipy(adj, device=DEV), args.reps))
    n, medges, _ = CONFIGS["arxiv-synth"][:3]
    ip, ix = uniform_graph(n, medges, SEEDS["arxiv-synth"], device=DEV)
    rows.append(measure("arxiv-synth", ppnp_amd.Graph.from_csr(ip, ix, None, n, device=DEV,
                                                               features=B), args.reps))
    for r in rows:
        r["chain_over_torch"] = r["chain_ms"] / r["torch_ms"]
        r["chain_over_solve"] = r["chain_ms"] / r["solve_ms"]
    info = ppnp_amd._lib.load().appnp_build_info().decode()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "topk_select.json"), "w") as fh:
        json.dump({"tool": "tools/topk_measure.py", "device": torch.cuda.get_device_name(0),
                   "library": info, "reps": args.reps, "results": rows}, fh, indent=1)
        fh.write("\n")
    print("topk_select.json", json.dumps(rows))


if __name__ == "__main__":
    main()
