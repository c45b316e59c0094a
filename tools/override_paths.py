"""Compare a rocprofv3 kernel trace of tests/override_worker.py with the launches that
tests/step_variants.py predicts (the worker's --trace-plan file).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tests/override_worker.py --set capped --out o.npz --trace-plan plan.json
    python tools/override_paths.py LABEL plan.json DIR

The k_step_* dispatches of the trace (k_rem_persist for the source-block set), in dispatch
order, must be the plan's kernels with the plan's grids (blocks = Grid_Size / Workgroup_Size).
Prints one line per case and exits 1 on a mismatch.
"""
import csv
import glob
import json
import os
import re
import sys


def main():
    label, plan_path, trace_dir = sys.argv[1:4]
    plan = json.load(open(plan_path))
    family = "k_rem_persist" if plan and plan[0]["kernel"].startswith("k_rem_persist") else "k_step_"
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for path in paths:
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    seen = []
    for r in rows:
        m = re.search(r"(k_step_(?:wide|narrow)|k_rem_persist)<[^>]*>", r["Kernel_Name"])
        if m and m.group(0).startswith(family):
            seen.append((m.group(0), [int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]),
                                      int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"])]))
    print(f"== {label}: {len(plan)} launches predicted, {len(seen)} {family}* dispatches traced")
    bad = len(plan) != len(seen)
    last = None
    for want, got in zip(plan, seen):
        grid_ok = want["grid"][0] is None or want["grid"] == got[1]
        ok = want["kernel"] == got[0] and grid_ok
        bad |= not ok
        line = (f"{want['case']:44s} predicted {want['kernel']} grid {want['grid']} | traced "
                f"{got[0]} grid {got[1]} {'ok' if ok else 'MISMATCH'}")
        if line != last:  # the launches of a case repeat: print each distinct line once
            print(line)
        last = line
    print(f"== {label}: {'MISMATCH' if bad else 'all predictions matched'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
