"""Times of the NNI climb under -bb (mpf_ufboot_optimize_nni) next to the plain climb (mpf_optimize_nni), DESIGN §5j.

    python tools/nni_bb_timing.py --out profiles/nni_bb_timing.json          # wall times, C2 and C3
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/nni_bb_timing.py --kernels C2 C3
                                                                              # k_nni_eval / k_nni_eval_masks per launch: the
                                                                              # *_kernel_stats.csv under DIR

--kernels runs nothing but full evaluations (the plain kernel through nni_scores, the mask-writing one through
nni_pattern_terms), 20 of each per workload, so that the two kernels' rows of the stats file are one full evaluation each.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpboot_amd import engine, synth, trees  # noqa: E402


def load(wl):
    letters, _ = synth.workload(wl)
    codes = synth.letters_to_codes(letters, "DNA")
    e = engine.FitchEngine(codes)
    e.stepwise_addition(7)
    return codes, e, e.get_tree()


def kernels(workloads):
    for wl in workloads:
        _codes, e, start = load(wl)
        for _ in range(20):
            e.nni_scores(1)
        for _ in range(20):
            e.nni_pattern_terms(1)


def spread(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)), "runs": len(ts)}


def wall(workloads, n_samples, out_path):
    out = {}
    for wl in workloads:
        codes, e, start = load(wl)
        n, P = codes.shape
        r = {"n": n, "Wp": e.Wp, "samples": n_samples}

        def timed(fn, k):
            ts = []
            for _ in range(k):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return ts

        e.nni_scores(1)
        r["plain_full_eval_ms"] = spread(timed(lambda: e.nni_scores(1), 15))
        rnd = trees.random_topology(n, np.random.default_rng(5))
        res = None

        def plain_climb():
            nonlocal res
            e.set_tree(rnd)
            t0 = time.perf_counter()
            res = e.optimize_nni(1, True)
            return (time.perf_counter() - t0) * 1e3

        plain_climb()
        r["plain_climb_random_ms"] = spread([plain_climb() for _ in range(5)])
        r["plain_climb_result"] = list(res)
        samples = np.random.default_rng(7).multinomial(P, np.ones(P) / P, size=n_samples).astype(np.uint16)
        e.seed_ties(engine.TIE_RANDOM, 5)
        e.ufboot_attach(samples)

        def tracked(tree, speednni, steps):
            e.set_tree(tree)
            b0 = e.get_option("nni_booked")
            t0 = time.perf_counter()
            rr = e.ufboot_optimize_nni(1, speednni, steps)
            return (time.perf_counter() - t0) * 1e3, rr, e.get_option("nni_booked") - b0

        # one scoring step of the whole tree on the stepwise tree: launch + R_T + product + extraction + replay (+ the step's
        # swaps and refresh when it finds moves)
        tracked(start, False, 1)
        one = [tracked(start, False, 1) for _ in range(7)]
        r["tracked_one_step_ms"] = spread([t for t, _r, _b in one])
        r["tracked_one_step_booked"] = one[-1][2]
        tr = [tracked(rnd, True, 50) for _ in range(3)]
        r["tracked_climb_random_ms"] = spread([t for t, _r, _b in tr])
        r["tracked_climb_result"] = list(tr[-1][1])
        r["tracked_climb_booked"] = tr[-1][2]
        r["same_climb"] = list(tr[-1][1]) == list(res)
        e.ufboot_detach()
        plain_climb()
        r["plain_climb_random_after_ms"] = spread([plain_climb() for _ in range(5)])
        out[wl] = r
        print(wl, json.dumps(r), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


def rules(workloads, n_samples, rule_names, out_path):
    """--rule: per workload ONE tracked climb from the tool's random tree under each named rule (option nni_tracked_rules), the
    default rule timed next to it in the same run; a fresh tracker per climb, so that every climb books into empty lists"""
    out = {}
    for wl in workloads:
        codes, e, _start = load(wl)
        n, P = codes.shape
        e.set_option("nni_tracked_rules", 1)
        rnd = trees.random_topology(n, np.random.default_rng(5))
        samples = np.random.default_rng(7).multinomial(P, np.ones(P) / P, size=n_samples).astype(np.uint16)
        r = {"n": n, "Wp": e.Wp, "samples": n_samples}
        for name in ["default"] + [x for x in rule_names if x != "default"]:
            ts = []
            for _ in range(3):
                e.seed_ties(engine.TIE_RANDOM, 5)
                e.ufboot_attach(samples)
                if name == "storetrees":
                    e.ufboot_set_store_trees(True)
                elif name == "topboot":
                    e.ufboot_set_mulhits(True)
                    e.ufboot_set_topboot(10)
                elif name == "distinct":
                    e.ufboot_set_distinct_iter(2)
                    e.ufboot_set_iteration(1)
                e.set_tree(rnd)
                b0 = e.get_option("nni_booked")
                t0 = time.perf_counter()
                res = e.ufboot_optimize_nni(1, True, 50)
                ts.append((time.perf_counter() - t0) * 1e3)
                booked = e.get_option("nni_booked") - b0
                dups = e.ufboot_duplicates()
                e.ufboot_detach()
            r[name] = {"tracked_climb_random_ms": spread(ts), "result": list(res), "booked": booked, "duplicates": dups}
        for name in r:
            if isinstance(r[name], dict) and name != "default":
                r[name]["ratio_to_default"] = r[name]["tracked_climb_random_ms"]["median"] / r["default"]["tracked_climb_random_ms"]["median"]
        out[wl] = r
        print(wl, json.dumps(r), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rule", nargs="*", default=None, choices=["default", "storetrees", "topboot", "distinct"],
                    help="one tracked climb per named rule next to the default rule (no name: all of them)")
    ap.add_argument("--kernels", nargs="*", default=None, help="only full evaluations by both kernels (for a kernel trace)")
    ap.add_argument("--workloads", nargs="*", default=["C2", "C3"])
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernels is not None:
        kernels(a.kernels or ["C2", "C3"])
    elif a.rule is not None:
        rules(a.workloads, a.samples, a.rule or ["storetrees", "topboot", "distinct"], a.out)
    else:
        wall(a.workloads, a.samples, a.out)
