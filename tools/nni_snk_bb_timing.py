"""Times of the weighted NNI climb under -bb (mpf_ufboot_optimize_nni on a weighted engine, k_snk_nni_eval_vals) next to the plain
weighted kernel and climb (k_snk_nni_eval, mpf_optimize_nni), DESIGN §5j.

    python tools/nni_snk_bb_timing.py --out profiles/nni_snk_bb_timing.json          # C2 and C5, 1000 samples

Per workload, in one process, under a symmetric metric matrix and from one random topology:
  * k_snk_nni_eval_vals next to k_snk_nni_eval per full evaluation: HIP events around the launch inside the engine (option
    "timing", read-only option "nni_kernel_ns"), 5 launches of warm-up, then the mean of `--launches` (at least 20);
  * one tracked full evaluation (a climb capped at one step: launch, bit planes, product, extraction, replay, and the step's swaps
    and refresh when it finds moves) with the product's HIP-event time (reps_kernel_ms of ufboot_counters);
  * the tracked climb to its end next to the untracked one.
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


def spread(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)), "runs": len(ts)}


def per_launch_us(e, fn, launches):
    for _ in range(5):
        fn()
    t0 = e.get_option("nni_kernel_ns")
    for _ in range(launches):
        fn()
    return (e.get_option("nni_kernel_ns") - t0) / launches / 1e3


def run(workloads, n_samples, launches, out_path):
    out = {}
    for wl in workloads:
        cfg = synth.WORKLOADS[wl]
        letters, _ = synth.workload(wl)
        codes = synth.letters_to_codes(letters, cfg["alphabet"])
        protein = cfg["alphabet"] == "AA"
        S = 20 if protein else 4
        n, P = codes.shape
        rnd = trees.random_topology(n, np.random.default_rng(5))
        e = engine.FitchEngine(codes, datatype=engine.AA if protein else engine.DNA, cost=metric(S))
        for key in ("timing", "nni_weighted", "nni_weighted_tracked"):
            e.set_option(key, 1)
        e.set_tree(rnd)
        r = {"n": n, "kept_patterns": e.num_informative, "branches": n - 3, "samples": n_samples, "launches": launches}
        plain = per_launch_us(e, lambda: e.nni_scores(1), launches)
        vals = per_launch_us(e, lambda: e.nni_pattern_lengths(1), launches)      # (the event pair brackets the scoring kernel alone)
        r["k_snk_nni_eval_us"] = plain
        r["k_snk_nni_eval_vals_us"] = vals
        r["kernel_ratio"] = vals / plain if plain else None
        r["byte_ratio_arithmetic"] = (4 * S * 2 + 2 * 2) / (4 * S * 2)           # four loads of S 16-bit rows + two 16-bit row stores
        res = None

        def plain_climb():
            nonlocal res
            e.set_tree(rnd)
            t0 = time.perf_counter()
            res = e.optimize_nni(1, True)
            return (time.perf_counter() - t0) * 1e3

        plain_climb()
        r["plain_climb_random_ms"] = spread([plain_climb() for _ in range(3)])
        r["plain_climb_result"] = list(res)
        samples = np.random.default_rng(7).multinomial(P, np.ones(P) / P, size=n_samples).astype(np.uint16)
        e.seed_ties(engine.TIE_RANDOM, 5)
        e.ufboot_attach(samples)

        def tracked(steps):
            e.set_tree(rnd)
            b0, g0 = e.get_option("nni_booked"), e.ufboot_counters()["reps_kernel_ms"]
            t0 = time.perf_counter()
            rr = e.ufboot_optimize_nni(1, True, steps)
            return (time.perf_counter() - t0) * 1e3, rr, e.get_option("nni_booked") - b0, e.ufboot_counters()["reps_kernel_ms"] - g0

        tracked(1)
        one = [tracked(1) for _ in range(5)]
        r["tracked_one_step_ms"] = spread([t for t, _r, _b, _g in one])
        r["tracked_one_step_gemm_ms"] = spread([g for _t, _r, _b, g in one])
        r["tracked_one_step_booked"] = one[-1][2]
        tr = [tracked(50) for _ in range(3)]
        r["tracked_climb_random_ms"] = spread([t for t, _r, _b, _g in tr])
        r["tracked_climb_gemm_ms"] = spread([g for _t, _r, _b, g in tr])
        r["tracked_climb_result"] = list(tr[-1][1])
        r["tracked_climb_booked"] = tr[-1][2]
        r["same_climb"] = list(tr[-1][1]) == list(res)
        e.ufboot_detach()
        e.close()
        out[wl] = r
        print(wl, json.dumps(r), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["C2", "C5"])
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a.workloads, a.samples, max(20, a.launches), a.out)
