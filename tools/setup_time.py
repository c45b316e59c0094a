#!/usr/bin/env python
"""Host + device time of one graph set-up: Graph.from_scipy(adj, features=F, transpose=True) on a
synthetic workload, adjacency on the host, in 'sym' mode (degrees, A_hat, heavy rows, the
source-blocked copy) and in 'rw' mode (the same plus A_hat^T: the transpose and its heavy rows).
arxiv-synth is the smallest configuration where set-up is more than launch latency.  Prints one
JSON line: the median wall time of each, synchronised, after one warm-up.

    python tools/setup_time.py [--workload arxiv-synth] [--features 100] [--reps 9]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="arxiv-synth")
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()

    import ppnp_amd
    from ppnp_amd import _lib, synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ip, ix = synth.graph_for(args.workload, device="cpu")
    n = ip.numel() - 1
    adj = sp.csr_matrix((np.ones(ix.numel(), dtype=np.float32), ix.numpy(), ip.numpy()),
                        shape=(n, n))
    out = {"workload": args.workload, "n": n, "nnz": int(adj.nnz), "features": args.features,
           "reps": args.reps, "library": _lib.load().appnp_build_info().decode()}
    for mode in ("sym", "rw"):
        times = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = ppnp_amd.Graph.from_scipy(adj, mode=mode, device=dev, features=args.features,
                                          transpose=True)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            sb = g.source_block_bytes()
            del g
        ts = sorted(times[1:])
        out[f"from_scipy_{mode}_ms"] = 1e3 * ts[len(ts) // 2]
        out[f"from_scipy_{mode}_min_ms"] = 1e3 * ts[0]
        out[f"source_block_bytes_{mode}"] = int(sb)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
