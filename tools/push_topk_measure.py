#!/usr/bin/env python3
"""Measure the top k straight from the push's lists (appnp_push_topk, select="lists") against the
block route it replaces (appnp_push_columns + appnp_topk_columns, chunks of 128 sources).

Writes profiles/push_topk.json.  Per workload -- the Cora-ML fixture and arxiv-synth (169 k nodes;
with --products also products-synth, 2.45 M) -- 'sym', alpha = 0.1, k = 128, per eps in
{1e-4, 1e-5}, both routes in the same process, medians of --reps runs:

  call128        128 sources in one call of each route: device time between two events, per
                 source, and the lists route's launches under the per-launch timer
                 (ops.kernel_times: "push" is the one launch with push, selection and clean-up,
                 "copy" the clear and the thresholds).  128 slots: a slot's last source is not
                 cleaned up, so this call runs no clean-up at all
  all            every node as a source (arxiv-synth; Cora-ML too): ONE call of the lists route
                 (default slots) against the block route's loop over chunks of 128, per source
  cleanup        the clean-up's share of the push launch, from single-workgroup launches: 16
                 sources one after another on ONE slot (15 clean-ups) against the same sources as
                 16 calls of one source each (no clean-up), kernel times of the "push" launch:
                 share = (T_seq - sum T_alone) / T_seq * 16 / 15
  identical      the two routes' indices, value bits, rounds and left agree (they must)

Usage: python tools/push_topk_measure.py [--out DIR] [--reps N] [--products]
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
ALPHA, B, K, SEQ = 0.1, 128, 128, 16


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


def kernel_ms(fn, reps, launches=16):
    """Medians of the summed "push" and "copy" launches of fn, and the launch count."""
    split = {"push": [], "copy": []}
    for _ in range(reps + 1):
        t = ops.kernel_times(fn, torch.device(DEV), launches)
        for kind in split:
            split[kind].append(sum(ms for k, ms in t if k == kind))
    return {k: statistics.median(v[1:]) for k, v in split.items()}, len(t)


def block_route(G, idx, eps, chunk=B):
    out = []
    for s in range(0, int(idx.numel()), chunk):
        X, rounds, left = ops.push_columns(G, idx[s:s + chunk], ALPHA, eps)
        i, v = ops.topk_columns(X, K)
        out.append((i, v, rounds, left))
    return tuple(torch.cat([o[j] for o in out]) for j in range(4))


def identical(a, b):
    return bool(torch.equal(a[0], b[0])
                and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
                and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]))


def measure(name, G, reps, all_sources):
    n = G.n
    src = np.sort(np.random.default_rng(0).choice(n, B, replace=False))
    idx = torch.from_numpy(src).to(DEV)
    rows = []
    for eps in (1e-4, 1e-5):
        lists = lambda: ops.push_topk(G, idx, K, ALPHA, eps, slots=B)  # noqa: E731
        block = lambda: block_route(G, idx, eps)  # noqa: E731
        got, want = lists(), block()
        row = {"workload": name, "nodes": n, "nnz_hat": G.nnz_hat, "k": K, "eps": eps,
               "identical": identical(got, want),
               "rounds_max": int(got[2].max()), "left_max": int(got[3].max())}
        lists_ms, block_ms = wall_ms(lists, reps), wall_ms(block, reps)
        km, launches = kernel_ms(lists, reps)
        bkm, blaunches = kernel_ms(block, reps, 32)
        row["call128"] = {"sources": B, "slots": B, "lists_ms": lists_ms, "block_ms": block_ms,
                          "lists_us_per_source": 1e3 * lists_ms / B,
                          "block_us_per_source": 1e3 * block_ms / B,
                          "lists_over_block": lists_ms / block_ms,
                          "lists_kernel_ms": km, "lists_launches": launches,
                          "block_kernel_ms": bkm, "block_launches": blaunches}
        # the clean-up's share: SEQ sources one after another on ONE slot (SEQ - 1 clean-ups)
        # against the same sources as SEQ calls of one source each (none)
        seq = kernel_ms(lambda: ops.push_topk(G, idx[:SEQ], K, ALPHA, eps, slots=1),
                        reps)[0]["push"]
        alone = sum(kernel_ms(lambda: ops.push_topk(G, idx[i:i + 1], K, ALPHA, eps, slots=1),
                              reps)[0]["push"] for i in range(SEQ))
        row["cleanup"] = {"sources": SEQ, "push_ms_one_slot": seq, "push_ms_one_call_each": alone,
                          "cleanups": SEQ - 1,
                          "share_of_push_launch": (seq - alone) / seq * SEQ / (SEQ - 1)}
        if all_sources:
            every = torch.arange(n, device=DEV)
            slots = ops.push_topk_slots(G, n)
            lists_all = lambda: ops.push_topk(G, every, K, ALPHA, eps)  # noqa: E731
            block_all = lambda: block_route(G, every, eps)  # noqa: E731
            same = identical(lists_all(), block_all())
            la, ba = wall_ms(lists_all, reps), wall_ms(block_all, reps)
            lib = ppnp_amd._lib.load()
            row["all"] = {"sources": n, "slots": slots, "identical": same, "lists_ms": la,
                          "block_ms": ba, "lists_us_per_source": 1e3 * la / n,
                          "block_us_per_source": 1e3 * ba / n, "lists_over_block": la / ba,
                          "lists_workspace_bytes":
                              int(lib.appnp_push_topk_workspace_bytes(n, slots)),
                          "block_workspace_bytes": int(lib.appnp_push_workspace_bytes(n, B))
                          + int(lib.appnp_topk_workspace_bytes(n, B, K)) + 4 * n * B}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def synth(name):
    n, medges, _ = CONFIGS[name][:3]
    ip, ix = uniform_graph(n, medges, SEEDS[name], device=DEV)
    return ppnp_amd.Graph.from_csr(ip, ix, None, n, device=DEV, features=B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--products", action="store_true",
                    help="also products-synth (2.45 M nodes), the 128-source call only")
    args = ap.parse_args()
    g = np.load(os.path.join(ROOT, "tests", "golden", "cora_ml.npz"), allow_pickle=False)
    n = int(g["n"])
    adj = sp.csr_matrix((g["adj_data"], g["adj_indices"], g["adj_indptr"]), shape=(n, n))
    rows = measure("cora-ml-real", ppnp_amd.Graph.from_scipy(adj, device=DEV), args.reps, True)
    rows += measure("arxiv-synth", synth("arxiv-synth"), args.reps, True)
    if args.products:
        rows += measure("products-synth", synth("products-synth"), args.reps, False)
    info = ppnp_amd._lib.load().appnp_build_info().decode()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "push_topk.json"), "w") as fh:
        json.dump({"tool": "tools/push_topk_measure.py", "device": torch.cuda.get_device_name(0),
                   "library": info, "reps": args.reps, "alpha": ALPHA, "mode": "sym", "k": K,
                   "results": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
