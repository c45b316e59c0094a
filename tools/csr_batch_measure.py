#!/usr/bin/env python3
"""Measure the device minibatch slice (ops.csr_batch, ``SparsePPR.batch(idx, slicer="device")``)
against the torch route it stands beside.  Writes profiles/csr_batch.json.

  slice     per matrix and batch size b in {128, 1024}: host wall time of one batch slice, from
            the call to the end of a device synchronise (the routes differ in host
            synchronisations, which device events alone would not show), median of --reps
            batches, the two routes alternating on the same batches.  The torch route's time
            includes the ``transpose()`` that the backward of ``sparse_linear`` would force
            (``appnp_csr_transpose``); the device route arrives with it.  Also: the device
            route's launches per batch with the time of each from the per-launch timer
            (ops.kernel_times), the device-side launches and copies of either route as
            torch.profiler counts them (null where the profiler is not available), and whether
            the two routes' outputs are identical (they must be).
            Matrices: the Cora-ML ``sparsified_ppr(k=128)``; arxiv-synth
            ``sparsified_ppr(k=128, eps=1e-4, select="lists")``; with --products the
            ``topk_rows`` of 4096 sources of products-synth (2.45 M columns; the full matrix is
            not built).
  trainer   ``python -m ppnp_amd.train --dataset cora_ml --n-runs 5 --batch-size 128 --ppr-topk
            128`` in a child process: in --parent-tree (a built checkout of the parent commit)
            when given, else on this tree with the default slicer; and on this tree with
            ``--batch-slice device``.  Per command: valid_acc per run, s/run (the training loop's
            time up to the best epoch), ms per epoch.

Usage: python tools/csr_batch_measure.py [--out DIR] [--reps N] [--products]
                                         [--parent-tree DIR] [--no-trainer]
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
from ppnp_amd import ops  # noqa: E402
from ppnp_amd.ppr import SparsePPR, sparsified_ppr, topk_rows  # noqa: E402
from ppnp_amd.synth import CONFIGS, SEEDS, uniform_graph  # noqa: E402

DEV = "cuda:0"
K = 128
COUNT_LAUNCHES = ("clear", "mark", "rows", "scan")
EMIT_LAUNCHES = ("sel", "emit", "tscan", "scatter", "sort")
TRAIN = ["-m", "ppnp_amd.train", "--dataset", "cora_ml", "--n-runs", "5", "--batch-size", "128",
         "--ppr-topk", "128"]


def torch_route(P, idx):
    sub, sel = P.batch(idx)
    sub.transpose()  # what the backward of sparse_linear would force
    return sub, sel


def device_route(P, idx):
    return P.batch(idx, slicer="device")


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def device_events(fn):
    """(kernel launches, copies) on the device during fn, by torch.profiler; None if it fails."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = copies = 0
        for ev in prof.events():
            if str(ev.device_type).endswith("CUDA"):
                name = ev.name.lower()
                if "memcpy" in name or "copy" in name and "kernel" not in name:
                    copies += 1
                else:
                    kernels += 1
        return {"kernels": kernels, "copies": copies} if kernels else None
    except Exception as e:  # measurement aid only
        print(f"torch.profiler not usable: {e}", file=sys.stderr)
        return None


def same(a, b):
    (sa, la), (sb, lb) = a, b
    ta, tb = sa.transpose(), sb.transpose()
    pairs = [(sa.indptr, sb.indptr), (sa.indices, sb.indices),
             (sa.data.view(torch.int32), sb.data.view(torch.int32)), (la, lb), (ta[0], tb[0]),
             (ta[1], tb[1]), (ta[2].view(torch.int32), tb[2].view(torch.int32))]
    return all(torch.equal(x, y) for x, y in pairs)


def measure_slice(name, P, reps):
    rows = []
    n_rows = P.shape[0]
    rng = np.random.default_rng(0)
    for b in (128, 1024):
        if b > n_rows:
            continue
        batches = [torch.from_numpy(rng.choice(n_rows, b, replace=False)).to(DEV)
                   for _ in range(reps + 2)]
        identical = same(torch_route(P, batches[0]), device_route(P, batches[0]))
        t_ms, d_ms = [], []
        for idx in batches:  # alternating; the first two batches warm both routes up
            t_ms.append(wall_ms(lambda: torch_route(P, idx)))
            d_ms.append(wall_ms(lambda: device_route(P, idx)))
        t_med, d_med = statistics.median(t_ms[2:]), statistics.median(d_ms[2:])
        kt = [ops.kernel_times(lambda: device_route(P, idx), torch.device(DEV), 32)
              for idx in batches[2:]]
        names = COUNT_LAUNCHES + EMIT_LAUNCHES
        per = {nm: statistics.median(r[i][1] for r in kt) for i, nm in enumerate(names)
               if all(len(r) == len(names) for r in kt)}
        sub, sel = device_route(P, batches[2])
        row = {"matrix": name, "rows": n_rows, "cols": P.shape[1], "nnz": P.nnz, "b": b,
               "kept_entries": sub.nnz, "n_sel": int(sel.numel()), "identical": identical,
               "torch_ms": t_med, "device_ms": d_med, "device_over_torch": d_med / t_med,
               "torch_ms_min_max": [min(t_ms[2:]), max(t_ms[2:])],
               "device_ms_min_max": [min(d_ms[2:]), max(d_ms[2:])],
               "device_library_launches": len(kt[0]),
               "device_launch_ms": per, "device_launch_ms_sum": sum(per.values()),
               "torch_device_events": device_events(lambda: torch_route(P, batches[3])),
               "device_device_events": device_events(lambda: device_route(P, batches[3]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def synth(name):
    n, medges, _ = CONFIGS[name][:3]
    ip, ix = uniform_graph(n, medges, SEEDS[name], device=DEV)
    return ppnp_amd.Graph.from_csr(ip, ix, None, n, device=DEV, features=K)


def run_trainer(tree, extra):
    env = dict(os.environ, PYTHONPATH=tree)
    t = time.perf_counter()
    out = subprocess.run([sys.executable] + TRAIN + extra, cwd=tree, env=env, check=True,
                         capture_output=True, text=True).stdout
    wall = time.perf_counter() - t
    s = json.loads(out.strip().splitlines()[-1])
    recs = s["records"]
    return {"tree": "parent" if tree != ROOT else "this",
            "command": "python " + " ".join(TRAIN + extra),
            "valid_acc": [r["valid_acc"] for r in recs],
            "valid_acc_mean": s["valid_acc_mean"], "best_epoch_mean": s["epochs_mean"],
            "s_per_run": s["elapsed_mean"],
            "ms_per_epoch": 1e3 * statistics.mean(r["elapsed"] / (r["epoch"] + 1) for r in recs),
            "ppr_build_mean_s": s["ppr_build_mean"], "process_wall_s": wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--products", action="store_true",
                    help="also topk_rows of 4096 sources of products-synth (2.45 M columns)")
    ap.add_argument("--parent-tree", default=None,
                    help="a built checkout of the parent commit for the trainer's baseline")
    ap.add_argument("--no-trainer", action="store_true")
    args = ap.parse_args()
    g = np.load(os.path.join(ROOT, "tests", "golden", "cora_ml.npz"), allow_pickle=False)
    n = int(g["n"])
    adj = sp.csr_matrix((g["adj_data"], g["adj_indices"], g["adj_indptr"]), shape=(n, n))
    G = ppnp_amd.Graph.from_scipy(adj, device=DEV)
    rows = measure_slice("cora-ml sparsified_ppr(k=128)", sparsified_ppr(G, K), args.reps)
    G = synth("arxiv-synth")
    rows += measure_slice("arxiv-synth sparsified_ppr(k=128, eps=1e-4, select='lists')",
                          sparsified_ppr(G, K, eps=1e-4, select="lists"), args.reps)
    if args.products:
        G = synth("products-synth")
        src = torch.from_numpy(np.sort(np.random.default_rng(1).choice(G.n, 4096, replace=False)))
        P = topk_rows(G, src.to(DEV), K, eps=1e-4, select="lists")
        rows += measure_slice("products-synth topk_rows(4096 sources, k=128, eps=1e-4, "
                              "select='lists')", P, args.reps)
    del G
    torch.cuda.empty_cache()
    trainer = []
    if not args.no_trainer:
        base = args.parent_tree or ROOT
        # twice each, alternating: the spread of the same command beside the difference
        for _ in range(2):
            trainer.append(run_trainer(os.path.abspath(base), []))
            trainer.append(run_trainer(ROOT, ["--batch-slice", "device"]))
        for t in trainer:
            print(json.dumps(t), flush=True)
    info = ppnp_amd._lib.load().appnp_build_info().decode()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "csr_batch.json"), "w") as fh:
        json.dump({"tool": "tools/csr_batch_measure.py", "device": torch.cuda.get_device_name(0),
                   "library": info, "reps": args.reps, "k": K,
                   "device_launch_names": list(COUNT_LAUNCHES + EMIT_LAUNCHES),
                   "slice": rows, "trainer": trainer}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
