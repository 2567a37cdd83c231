"""Times of the TBR sweep under -bb on the weighted (-cost) engine (mpf_ufboot_tbr_sweep under "tbr_weighted_tracked",
k_tbr_snk_vals) next to the plain weighted sweep (mpf_tbr_sweep_best under "tbr_weighted"), DESIGN 5q.

    python tools/tbr_snk_bb_timing.py --out profiles/tbr/timing_weighted_tracked.json

One MI355X, 1000 samples, the 16-bit store.  Synth C2 (200 x 10 000 DNA) under tstv at radius 3 and radius 6 and C5 (500 x 20 000
protein) under a 20 x 20 metric at radius 3, a random tree each, without a cut-off and under a logl_cutoff at the top 10 % of the first
sweep's lengths.  Every figure: two warm-ups, then median [min .. max] of 7 whole calls.  Every (workload, radius) is a child process
of its own under `timeout`, one GPU process at a time; a step that fails ends the run, what was measured until then is kept.
Nothing comparable exists without this option (the parent refuses the call), so no ratio is fixed in advance.

Per run, in ONE process:
  plain_before / plain_after   mpf_tbr_sweep_best before the attach and after the last detach
  tracked                      mpf_ufboot_tbr_sweep on a tracker attached afresh for every call (the attach is not timed): whole call,
                               trees handed over, trees booked, batches, tie draws, events; under the option "timing" in a second
                               pass the three timers: tbr_masks_ns (here k_tbr_snk_vals and the plane slicing), tbr_product_ns,
                               tbr_extract_ns
  tracked_spr                  (--spr, C2 only) a whole mpf_optimize_spr climb at the same radius from the same tree under a tracker
                               attached afresh, 1 warm-up and 3 calls: the weighted tracked SPR loop's trees booked per second.  That
                               loop has no visit cap ("max_visits" is a Fitch aid), so it is a climb and not one sweep's worth of
                               visits, and C5 is left out: a climb of 500 taxa from a random tree does not fit a step's limit
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (workload, matrix, alphabet, radius, seconds the step may take)
STEPS = [("C2", "tstv", "DNA", 3, 240), ("C2", "tstv", "DNA", 6, 300), ("C5", "metric20", "AA", 3, 420)]
WARM, REPS = 2, 7
TIMERS = ("tbr_masks_ns", "tbr_product_ns", "tbr_extract_ns")


def matrix(kind):
    if kind == "tstv":
        c = np.full((4, 4), 2, dtype=np.uint32)
        np.fill_diagonal(c, 0)
        c[0, 2] = c[2, 0] = c[1, 3] = c[3, 1] = 1
        return c
    pts = np.random.default_rng(4).integers(0, 12, size=(20, 3))     # Manhattan distances of random points: symmetric, closed
    c = np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2).astype(np.uint32)
    c[c == 0] = 1
    np.fill_diagonal(c, 0)
    return c


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def timed(fn):
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def step(shape, kind, alphabet, radius, n_samples, with_spr):
    from mpboot_amd import engine, synth, trees
    letters, _ = synth.workload(shape)
    codes = synth.letters_to_codes(letters, alphabet)
    n, P = codes.shape
    eng = engine.FitchEngine(codes, datatype=0 if alphabet == "DNA" else 1, cost=matrix(kind))
    eng.set_option("tbr_weighted", 1)
    eng.set_option("tbr_weighted_tracked", 1)
    eng.set_option("sankoff_short", 1)
    back = trees.random_topology(n, np.random.default_rng(1))
    samples = np.random.default_rng(7).multinomial(P, np.ones(P) / P, size=n_samples).astype(np.uint16)
    eng.seed_ties(engine.TIE_RANDOM, 5)
    length = eng.score_tree(back)
    out = {"taxa": int(n), "columns": int(P), "kept_patterns": int(eng.num_informative), "row_patterns_padded": int(eng.Wp), "matrix": kind,
           "store_bits": 16 if eng.get_option("sankoff_packed") else 32, "radius": radius, "samples": n_samples, "length": int(length),
           "warm_ups": WARM, "calls_per_figure": REPS}
    out["plain_before"] = spread(timed(lambda: eng.tbr_sweep_best(radius)))

    def tracked(cutoff, timing):
        """WARM + REPS calls, each on a tracker attached afresh -> the figures of the timed ones"""
        wall, info, split = [], {}, {"k_tbr_snk_vals_and_planes": [], "product": [], "extraction": []}
        eng.set_option("timing", 1 if timing else 0)
        for k in range(WARM + REPS):
            eng.set_tree(back)
            eng.ufboot_attach(samples)
            if cutoff:
                eng.ufboot_set_cutoff(cutoff)
            ns0 = [eng.get_option(o) for o in TIMERS]
            t0 = time.perf_counter()
            _c, _f, _g, pairs = eng.ufboot_tbr_sweep(radius)
            ms = (time.perf_counter() - t0) * 1e3
            if k >= WARM:
                wall.append(ms)
                for key, o, z in zip(split, TIMERS, ns0):
                    split[key].append((eng.get_option(o) - z) / 1e6)
            cnt = eng.ufboot_counters()
            info = {"pairs": int(pairs), "handed_over": int(eng.get_option("tbr_booked")), "booked": int(len(eng.ufboot_tree_logl())),
                    "batches": int(eng.get_option("tbr_book_batches")), "chunks": int(eng.get_option("tbr_chunks")),
                    "tie_draws": int(cnt["tie_draws"]), "events": int(cnt.get("events", 0))}
            logl = eng.ufboot_tree_logl()
            eng.ufboot_detach()
        eng.set_option("timing", 0)
        info["whole_call"] = spread(wall)
        if timing:
            info["timing"] = {k: spread(v) for k, v in split.items()}
        else:
            info["handed_over_per_s"] = info["handed_over"] / (statistics.median(wall) * 1e-3)
            info["booked_per_s"] = info["booked"] / (statistics.median(wall) * 1e-3)
        return info, logl

    def both(cutoff):
        res, logl = tracked(cutoff, False)
        res["under_option_timing"], _ = tracked(cutoff, True)
        return res, logl

    out["tracked_no_cutoff"], logl = both(0.0)
    cutoff = float(np.sort(np.asarray(logl))[int(len(logl) * 0.9)])          # the best 10 % of the first sweep's lengths pass
    out["cutoff"] = cutoff
    out["tracked_cutoff_top_10_percent"], _ = both(cutoff)

    # the weighted tracked SPR loop: a whole climb from the same tree at the same radius
    def spr(cut):
        wall, booked, warm, reps = [], 0, 1, 3
        for k in range(warm + reps):
            eng.set_tree(back)
            eng.seed_ties(engine.TIE_RANDOM, 5)
            eng.ufboot_attach(samples)
            if cut:
                eng.ufboot_set_cutoff(cut)
            t0 = time.perf_counter()
            eng.optimize_spr(1, radius)
            ms = (time.perf_counter() - t0) * 1e3
            if k >= warm:
                wall.append(ms)
            booked = int(len(eng.ufboot_tree_logl()))
            eng.ufboot_detach()
        return {"what": "a whole climb, 1 warm-up and 3 calls", "booked": booked, "whole_call": spread(wall),
                "booked_per_s": booked / (statistics.median(wall) * 1e-3)}

    if with_spr:
        out["tracked_spr_no_cutoff"] = spr(0.0)
        out["tracked_spr_cutoff_top_10_percent"] = spr(cutoff)
    else:
        out["tracked_spr_no_cutoff"] = out["tracked_spr_cutoff_top_10_percent"] = "not timed"
    eng.set_tree(back)
    eng.score_tree(back)
    out["plain_after"] = spread(timed(lambda: eng.tbr_sweep_best(radius)))
    print(json.dumps(out))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return None, r.returncode
    return json.loads(r.stdout.strip().splitlines()[-1]), 0


def save(res, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated workloads, e.g. C2")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--spr", action="store_true", help="time the weighted tracked SPR climb on C2 as well")
    ap.add_argument("--step", default=None, help="(child) workload,matrix,alphabet,radius")
    a = ap.parse_args()
    if a.step:
        shape, kind, alphabet, radius = a.step.split(",")
        step(shape, kind, alphabet, int(radius), a.samples, a.spr)
    else:
        res = {"protocol": "one MI355X, 16-bit store, %d samples, %d warm-ups, median [min .. max] of %d whole calls" % (a.samples, WARM, REPS),
               "workloads": {}}
        for shape, kind, alphabet, radius, limit in STEPS:
            if a.only and shape not in a.only.split(","):
                continue
            args = ["--step", "%s,%s,%s,%d" % (shape, kind, alphabet, radius), "--samples", str(a.samples)]
            if a.spr and shape == "C2":
                args.append("--spr")
            one, rc = child(args, limit)
            key = "%s_%s_radius_%d" % (shape, kind, radius)
            if rc:
                res["workloads"][key] = "not timed: the step ended with status %d within its limit of %d s" % (rc, limit)
                save(res, a.out)
                raise SystemExit("step %s ended with status %d: stopping here" % (key, rc))
            res["workloads"][key] = one
            save(res, a.out)
            print(json.dumps({key: one}), flush=True)
