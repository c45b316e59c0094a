#!/usr/bin/env python
"""Per-step device time of the polynomial propagation against the fixed-alpha one, from the
library's per-launch timer (ops.kernel_times), both sides in the same run on the same build:

    appnp_poly      against appnp_propagate       (epilogue POLY     against FWD)
    appnp_poly_bwd  against appnp_propagate_bwd   (POLY / POLY_DOT   against BWD),
                    without and with dcoef

on Cora-ML (the fixture, F = 7) and arxiv-synth (F = 128), K = 10.  Beside the measured ratios
it writes what the streams explain: per step and row, FWD reads H and writes Z (2 rows of F
floats), POLY reads Z and writes T_k and Z (3; the last step 2), BWD reads dH and writes G_k and
dH (3), POLY_DOT also reads H (4) and writes 4 slabs n bytes of partials; every step reads the
CSR (8 bytes an entry) and gathers nnz rows of F floats (an upper bound: the caches serve part).

    python tools/poly_step_cost.py [--reps 20] [--out profiles/poly_step_cost.json]
"""

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_us(fn, dev, reps):
    """Median over ``reps`` calls of (mean "step" launch, sum of the other launches), in us."""
    from ppnp_amd import ops

    fn()
    torch.cuda.synchronize()
    steps, rest = [], []
    for _ in range(reps):
        t = ops.kernel_times(fn, dev)
        s = [ms for kind, ms in t if kind == "step"]
        steps.append(1e3 * sum(s) / max(len(s), 1))
        rest.append(1e3 * sum(ms for kind, ms in t if kind != "step"))
    return statistics.median(steps), statistics.median(rest)


def measure(workload, reps):
    import ppnp_amd
    from ppnp_amd import ops, synth

    n, _, F, K, alpha, _ = synth.CONFIGS[workload]
    dev = torch.device("cuda", 0)
    indptr, indices = synth.graph_for(workload, device=dev)
    G = ppnp_amd.Graph.from_csr(indptr, indices, None, n, device=dev)
    H = synth.features(n, F, device=dev)
    dZ = synth.features(n, F, device=dev, seed=1)
    coef = ppnp_amd.ppr_coefficients(K, alpha, device=dev)
    calls = {
        "propagate": lambda: ops.propagate_forward(G, H, K, alpha),
        "poly": lambda: ops.poly_forward(G, H, coef),
        "propagate_bwd": lambda: ops.propagate_backward(G, dZ, K, alpha),
        "poly_bwd": lambda: ops.poly_backward(G, dZ, None, coef, need_dcoef=False),
        "poly_bwd_dcoef": lambda: ops.poly_backward(G, dZ, H, coef),
    }
    out = {"n": n, "nnz_hat": G.nnz_hat, "F": F, "K": K}
    for name, fn in calls.items():
        step, rest = step_us(fn, dev, reps)
        out[name] = {"step_us": round(step, 3), "other_launches_us": round(rest, 3)}
    # bytes a step moves when no gather hits a cache: CSR + gathers + streamed rows (+ partials)
    slabs = (F + 255) // 256  # 64 lanes of 4 floats
    base = G.nnz_hat * 8 + (n + 1) * 4 + G.nnz_hat * F * 4
    row = n * F * 4
    model = {"propagate": base + 2 * row, "poly": base + 3 * row, "propagate_bwd": base + 3 * row,
             "poly_bwd": base + 3 * row, "poly_bwd_dcoef": base + 4 * row + 4 * slabs * n}
    out["ratios"] = {}
    for a, b in (("poly", "propagate"), ("poly_bwd", "propagate_bwd"),
                 ("poly_bwd_dcoef", "propagate_bwd"), ("poly_bwd_dcoef", "poly_bwd")):
        out["ratios"][f"{a}/{b}"] = {
            "measured": round(out[a]["step_us"] / out[b]["step_us"], 4),
            "bytes_model": round(model[a] / model[b], 4)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_step_cost.json"))
    a = p.parse_args()
    import ppnp_amd

    res = {"device": torch.cuda.get_device_name(0),
           "build": ppnp_amd._lib.load().appnp_build_info().decode(), "reps": a.reps,
           "graphs": {w: measure(w, a.reps) for w in ("cora-ml-real", "arxiv-synth")}}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res["graphs"]))


if __name__ == "__main__":
    main()
