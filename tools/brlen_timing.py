"""Time of the branch-length kernels k_branch_subst / k_snk_branch_eval next to the NNI-scoring kernels, DESIGN §5k.

    python tools/brlen_timing.py --out profiles/brlen_timing.json              # C2, C3 (Fitch) and C5 weighted, 16-bit costs

Per workload one random topology, every branch of it (2 n - 3) per launch.  Recorded:
  * kernel time by HIP events around the launch inside the engine (option "timing", read-only option "brlen_kernel_ns"): 5
    evaluations of warm-up, then the mean of `--launches` (at least 20) evaluations;
  * wall time of branch_substitutions on valid views (the same evaluations);
  * wall time of branch_substitutions on a freshly set tree, the refresh of every view included (mean of 5);
  * in the same run, on the same tree, k_nni_eval / k_snk_nni_eval (one full evaluation, every inner branch, both moves) as the
    yardstick, and the ratio of the two kernel times.
`--only-fitch WL` runs the Fitch kernel of one workload alone, timing off (for a profiler run around the script).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpboot_amd import engine, synth, trees  # noqa: E402


def metric(S, seed=4):
    pts = np.random.default_rng(seed).integers(0, 12, size=(S, 3))
    c = np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2).astype(np.uint32)
    c[c == 0] = 1
    np.fill_diagonal(c, 0)
    return c


def measure(e, back, launches):
    e.set_option("timing", 1)
    e.set_tree(back)
    for _ in range(5):
        e.branch_substitutions(1)
    k0 = e.get_option("brlen_kernel_ns")
    t0 = time.perf_counter()
    for _ in range(launches):
        a, _b, _s = e.branch_substitutions(1)
    wall = (time.perf_counter() - t0) / launches
    kern = (e.get_option("brlen_kernel_ns") - k0) / launches
    fresh = 0.0
    for _ in range(5):
        e.set_tree(back)                               # the same tree handed over again: every vector stale
        t0 = time.perf_counter()
        e.branch_substitutions(1)
        fresh += (time.perf_counter() - t0) / 5
    for _ in range(5):
        e.nni_scores(1)
    n0 = e.get_option("nni_kernel_ns")
    for _ in range(launches):
        x, _y, _l = e.nni_scores(1)
    nni = (e.get_option("nni_kernel_ns") - n0) / launches
    return {"branches": len(a), "kernel_us": kern / 1e3, "wall_valid_views_us": wall * 1e6, "wall_fresh_tree_us": fresh * 1e6,
            "nni_branches": len(x), "nni_kernel_us": nni / 1e3, "kernel_over_nni_kernel": kern / nni if nni else None}


def run(launches, out_path):
    out = {}
    for wl, weighted in (("C2", False), ("C3", False), ("C5", True)):
        cfg = synth.WORKLOADS[wl]
        letters, _ = synth.workload(wl)
        codes = synth.letters_to_codes(letters, cfg["alphabet"])
        protein = cfg["alphabet"] == "AA"
        dt = engine.AA if protein else engine.DNA
        n = codes.shape[0]
        back = trees.random_topology(n, np.random.default_rng(5))
        if weighted:
            e = engine.FitchEngine(codes, datatype=dt, cost=metric(20 if protein else 4))
            e.set_option("nni_weighted", 1)
            kernel, yard = "k_snk_branch_eval_u16", "k_snk_nni_eval_u16"
            assert e.get_option("sankoff_short") == 1
        else:
            e = engine.FitchEngine(codes, datatype=dt)
            kernel, yard = "k_branch_subst", "k_nni_eval"
        r = {"n": n, "kept_patterns": e.num_informative, "launches": launches, "kernel": kernel, "yardstick": yard}
        r.update(measure(e, back, launches))
        # vectors loaded per launch: two per branch here; four per inner branch by the NNI kernels
        r["vectors_over_nni_vectors"] = 2 * (2 * n - 3) / (4 * (n - 3))
        e.close()
        out[wl + ("_weighted_u16" if weighted else "")] = r
        print(wl, json.dumps(r), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(out, fh, indent=1)


def only_fitch(wl, launches):
    cfg = synth.WORKLOADS[wl]
    letters, _ = synth.workload(wl)
    codes = synth.letters_to_codes(letters, cfg["alphabet"])
    e = engine.FitchEngine(codes, datatype=engine.AA if cfg["alphabet"] == "AA" else engine.DNA)
    e.set_tree(trees.random_topology(codes.shape[0], np.random.default_rng(5)))
    for _ in range(5 + launches):
        e.branch_substitutions(1)
    e.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fitch", default=None)
    a = ap.parse_args()
    if a.only_fitch:
        only_fitch(a.only_fitch, max(20, a.launches))
    else:
        run(max(20, a.launches), a.out)
