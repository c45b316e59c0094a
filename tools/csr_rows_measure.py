#!/usr/bin/env python3
"""Measure taking rows of a device CSR (ops.csr_rows: ``SparseFeatures.rows``,
``SparsePPR.rows(idx, slicer="device")``) against the torch route of ``SparsePPR.rows``.  Writes
profiles/csr_rows.json.

  rows      per matrix and index list: host wall time of one slice, from the call to the end of a
            device synchronise (the routes differ in host synchronisations, which device events
            alone would not show), median of --reps, the two routes alternating on the same
            ``idx`` and asserted bit-identical.  "with transpose": the device route emits it; the
            torch route's time includes the ``transpose()`` that a backward of ``sparse_linear``
            would force (``appnp_csr_transpose``).  "without": ``transpose=False`` against the
            torch route alone (a slice used under ``no_grad``).  Also the device route's launches
            with the time of each from the per-launch timer (ops.kernel_times).
            Matrices: the L1-normalised Cora-ML attribute matrix with the ``sel`` of b = 128 and
            b = 1024 minibatches of its ``sparsified_ppr(k=128)``; a seeded synthetic X over
            arxiv-synth's nodes (169,343 x 8192, 32 entries per row) with the ``sel`` of the same
            batch sizes of ``sparsified_ppr(k=128, eps=1e-4, select="lists")``; the Cora-ML
            ``sparsified_ppr(k=128)`` itself with 500 and 1500 rows (the stopping and validation
            sets).
  trainer   ``python -m ppnp_amd.train --dataset cora_ml --n-runs 5 --batch-size 128 --ppr-topk
            128 --batch-slice device`` with a dense X and with ``--sparse-x``, on this tree, each
            twice, alternating, in child processes.  Per command: valid_acc per run, s/run (the
            training loop's time up to the best epoch), ms per epoch.

Usage: python tools/csr_rows_measure.py [--out DIR] [--reps N] [--no-arxiv] [--no-trainer]
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ppnp_amd  # noqa: E402
from ppnp_amd import ops, train  # noqa: E402
from ppnp_amd.ppr import SparsePPR, sparsified_ppr  # noqa: E402
from ppnp_amd.synth import CONFIGS, SEEDS, uniform_graph  # noqa: E402

DEV = "cuda:0"
K = 128
LAUNCHES_T = ("count", "clear", "copy", "tscan", "scatter", "sort")
LAUNCHES = ("count", "copy")
TRAIN = ["-m", "ppnp_amd.train", "--dataset", "cora_ml", "--n-runs", "5", "--batch-size", "128",
         "--ppr-topk", "128", "--batch-slice", "device"]


def torch_route(M, idx, transpose):
    sub = M.rows(idx)
    if transpose:
        sub.transpose()  # what the backward of sparse_linear would force
    return sub


def device_route(M, idx, transpose):
    return M._rows_device(idx, transpose)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def same(a, b, transpose):
    pairs = [(a.indptr, b.indptr), (a.indices, b.indices),
             (a.data.view(torch.int32), b.data.view(torch.int32))]
    if transpose:
        ta, tb = a.transpose(), b.transpose()
        pairs += [(ta[0], tb[0]), (ta[1], tb[1]),
                  (ta[2].view(torch.int32), tb[2].view(torch.int32))]
    return all(torch.equal(x, y) for x, y in pairs)


def measure(name, M, what, idx, transpose, reps):
    """M: a SparsePPR (an attribute matrix is wrapped as one: the torch route lives there)."""
    t_ms, d_ms = [], []
    for _ in range(reps + 2):  # alternating; the first two calls warm both routes up
        t_ms.append(wall_ms(lambda: torch_route(M, idx, transpose)))
        d_ms.append(wall_ms(lambda: device_route(M, idx, transpose)))
    sub = device_route(M, idx, transpose)
    if not same(torch_route(M, idx, transpose), sub, transpose):
        raise AssertionError(f"{name}, {what}: the routes differ")
    names = LAUNCHES_T if transpose else LAUNCHES
    kt = [ops.kernel_times(lambda: device_route(M, idx, transpose), torch.device(DEV), 32)
          for _ in range(reps)]
    if not all(len(r) == len(names) for r in kt):
        raise AssertionError(f"{name}: {len(kt[0])} launches, expected {len(names)}")
    per = {nm: statistics.median(r[i][1] for r in kt) for i, nm in enumerate(names)}
    t_med, d_med = statistics.median(t_ms[2:]), statistics.median(d_ms[2:])
    row = {"matrix": name, "rows": M.shape[0], "cols": M.shape[1], "nnz": M.nnz, "idx": what,
           "b": int(idx.numel()), "transpose": transpose, "entries": sub.nnz, "identical": True,
           "torch_ms": t_med, "device_ms": d_med, "device_over_torch": d_med / t_med,
           "torch_ms_min_max": [min(t_ms[2:]), max(t_ms[2:])],
           "device_ms_min_max": [min(d_ms[2:]), max(d_ms[2:])],
           "device_launch_ms": per, "device_launch_ms_sum": sum(per.values())}
    print(json.dumps(row), flush=True)
    return row


def as_ppr(X):
    return SparsePPR(X.indptr, X.indices, X.data, X.shape, device=DEV)


def batch_sels(P, sizes, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for b in sizes:
        idx = torch.from_numpy(rng.choice(P.shape[0], b, replace=False)).to(DEV)
        out.append((f"sel of a b={b} batch", P.batch(idx, slicer="device")[1]))
    return out


def synth_x(n, f=8192, per_row=32, seed=7):
    """n x f CSR with ``per_row`` draws of a column per row (repeats removed), L1-normalised."""
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.integers(0, f, (n, per_row)), axis=1)
    keep = np.ones_like(cols, dtype=bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    X = sp.csr_matrix((rng.random(int(indptr[-1]), dtype=np.float32) + 0.1, cols[keep], indptr),
                      shape=(n, f))
    return sp.csr_matrix(train.normalize_attributes(X), dtype=np.float32)


def run_trainer(extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable] + TRAIN + extra, cwd=ROOT, env=env, check=True,
                         capture_output=True, text=True).stdout
    s = json.loads(out.strip().splitlines()[-1])
    recs = s["records"]
    return {"command": "python " + " ".join(TRAIN + extra),
            "valid_acc": [r["valid_acc"] for r in recs],
            "valid_acc_mean": s["valid_acc_mean"], "best_epoch_mean": s["epochs_mean"],
            "s_per_run": s["elapsed_mean"],
            "ms_per_epoch": 1e3 * statistics.mean(r["elapsed"] / (r["epoch"] + 1) for r in recs),
            "ppr_build_mean_s": s["ppr_build_mean"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--no-arxiv", action="store_true")
    ap.add_argument("--no-trainer", action="store_true")
    args = ap.parse_args()
    adj, attr, _ = train.load_dataset("cora_ml")
    G = ppnp_amd.Graph.from_scipy(adj, device=DEV)
    P = sparsified_ppr(G, K)
    X = as_ppr(ppnp_amd.SparseFeatures.from_scipy(train.normalize_attributes(attr), device=DEV))
    rows = []
    for what, sel in batch_sels(P, (128, 1024)):
        rows.append(measure("cora-ml attributes", X, what, sel, True, args.reps))
    rng = np.random.default_rng(1)
    for b in (500, 1500):
        idx = torch.from_numpy(rng.choice(P.shape[0], b, replace=False)).to(DEV)
        for transpose in (True, False):
            rows.append(measure("cora-ml sparsified_ppr(k=128)", P, f"{b} random rows", idx,
                                transpose, args.reps))
    if not args.no_arxiv:
        n, medges, _ = CONFIGS["arxiv-synth"][:3]
        ip, ix = uniform_graph(n, medges, SEEDS["arxiv-synth"], device=DEV)
        G = ppnp_amd.Graph.from_csr(ip, ix, None, n, device=DEV, features=K)
        P = sparsified_ppr(G, K, eps=1e-4, select="lists")
        X = as_ppr(ppnp_amd.SparseFeatures.from_scipy(synth_x(n), device=DEV))
        for what, sel in batch_sels(P, (128, 1024)):
            rows.append(measure("synthetic X over arxiv-synth (169,343 x 8192, 32 draws per row)",
                                X, what, sel, True, args.reps))
    del G, P, X
    torch.cuda.empty_cache()
    trainer = []
    if not args.no_trainer:
        for _ in range(2):  # twice each, alternating: the spread beside the difference
            trainer.append(run_trainer([]))
            trainer.append(run_trainer(["--sparse-x"]))
        for t in trainer:
            print(json.dumps(t), flush=True)
    info = ppnp_amd._lib.load().appnp_build_info().decode()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "csr_rows.json"), "w") as fh:
        json.dump({"tool": "tools/csr_rows_measure.py", "device": torch.cuda.get_device_name(0),
                   "library": info, "reps": args.reps, "k": K,
                   "device_launch_names": {"with transpose": list(LAUNCHES_T),
                                           "without": list(LAUNCHES)},
                   "rows": rows, "trainer": trainer}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
