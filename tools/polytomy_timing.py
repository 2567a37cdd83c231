"""Time of the multifurcating-tree views (k_poly_views) and the branch launch behind them, next to the binary engine, DESIGN §5l.

    python tools/polytomy_timing.py --out profiles/polytomy_timing.json        # C3: 1000 taxa x 50 000 DNA patterns

On one random binary topology of the workload, with HIP events inside the engine (option "timing"):
  * the tree with about a third of its inner branches contracted, and the star of the same taxa: the view launch (read-only option
    "poly_view_ns"), the branch launch ("poly_branch_ns"), the directed views written ("poly_views"), time per view;
  * the yardstick, the same visit: the binary tree handed over again (every vector stale), its whole-tree refresh
    (stats view_kernel_ms_total) and mpf_branch_substitutions' launch ("brlen_kernel_ns"), time per view over 3 (n - 2) views.
Five evaluations of warm-up, then the mean of `--launches` (at least 10).
`--only collapsed|star|binary` runs one of them alone, timing off (for a profiler run around the script).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpboot_amd import engine, synth, trees  # noqa: E402


def collapsed(back, n, rng, fraction):
    inner = [(v, int(back[3 * v + s]) // 3) for v in range(n + 1, 2 * n - 1) for s in range(3) if int(back[3 * v + s]) // 3 > v]
    return trees.collapse_branches(back, n, [br for br in inner if rng.random() < fraction])


def poly(e, first, nbr, launches):
    for _ in range(5):
        e.polytomy_branch_substitutions(first, nbr, 1)
    v0, b0, w0 = e.get_option("poly_view_ns"), e.get_option("poly_branch_ns"), e.get_option("poly_views")
    for _ in range(launches):
        a, _b, _s = e.polytomy_branch_substitutions(first, nbr, 1)
    view = (e.get_option("poly_view_ns") - v0) / launches
    views = (e.get_option("poly_views") - w0) // launches
    return {"inner_nodes": len(first) - 1, "max_degree": int(np.diff(first).max()), "branches": len(a), "views_written": int(views),
            "view_kernel_us": view / 1e3, "branch_kernel_us": (e.get_option("poly_branch_ns") - b0) / launches / 1e3,
            "ns_per_view": view / views}


def binary(e, back, n, launches):
    for _ in range(5):
        e.set_tree(back)
        e.branch_substitutions(1)
    v0, b0 = e.stats()["view_kernel_ms_total"], e.get_option("brlen_kernel_ns")
    for _ in range(launches):
        e.set_tree(back)                                   # the same tree handed over again: every vector stale
        e.branch_substitutions(1)
    view = (e.stats()["view_kernel_ms_total"] - v0) * 1e6 / launches
    return {"views_written": 3 * (n - 2), "view_kernel_us": view / 1e3, "branch_kernel_us": (e.get_option("brlen_kernel_ns") - b0) / launches / 1e3,
            "ns_per_view": view / (3 * (n - 2))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=("collapsed", "star", "binary"))
    a = ap.parse_args()
    launches = max(10, a.launches)
    letters, _ = synth.workload(a.workload)
    codes = synth.letters_to_codes(letters, synth.WORKLOADS[a.workload]["alphabet"])
    n = codes.shape[0]
    rng = np.random.default_rng(5)
    back = trees.random_topology(n, rng)
    third = collapsed(back, n, rng, 1 / 3)
    star = (np.array([0, n], dtype=np.int32), np.arange(1, n + 1, dtype=np.int32))
    e = engine.FitchEngine(codes, datatype=engine.DNA)
    if a.only:
        for _ in range(5 + launches):
            if a.only == "binary":
                e.set_tree(back)
                e.branch_substitutions(1)
            else:
                e.polytomy_branch_substitutions(*(third if a.only == "collapsed" else star), 1)
        sys.exit(0)
    e.set_option("timing", 2)
    out = {"workload": a.workload, "n": n, "kept_patterns": e.num_informative, "launches": launches,
           "collapsed_third": poly(e, *third, launches), "star": poly(e, *star, launches), "binary": binary(e, back, n, launches)}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
