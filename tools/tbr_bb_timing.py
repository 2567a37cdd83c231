"""Times of the TBR sweep under -bb (mpf_ufboot_tbr_sweep, k_tbr_masks) next to the plain sweep (mpf_tbr_sweep_best), DESIGN 5q.

    python tools/tbr_bb_timing.py --out profiles/tbr/timing_tracked.json

One MI355X, 1000 samples.  Synth C2 (200 x 10 000 DNA), a random tree, radius 3 and radius 6, without a cut-off and under a
logl_cutoff at the top 10 % of the first sweep's lengths.  Every figure: two warm-ups, then median [min .. max] of 7 whole calls.
Every (shape, radius) is a child process of its own under `timeout`, one GPU process at a time; a step that fails ends the run.
Nothing comparable exists without this entry point (the plain entries refuse a tracker), so no ratio is fixed in advance.

Per run, in ONE process:
  plain_before / plain_after   mpf_tbr_sweep_best before the attach and after the last detach
  tracked                      mpf_ufboot_tbr_sweep on a tracker attached afresh for every call (the attach is not timed): whole call,
                               trees handed over, trees booked, batches, tie draws, events; under the option "timing" in a second
                               pass the k_tbr_masks, product and extraction times (tbr_masks_ns, tbr_product_ns, tbr_extract_ns)
  tracked_spr                  the first 2 n - 2 prune-node visits (option "max_visits") of mpf_optimize_spr at the same radius on the
                               same tree under a tracker attached afresh: the tracked SPR loop's trees booked per second
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

RADII = (3, 6)
WARM, REPS = 2, 7


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


def step(shape, radius, n_samples):
    from mpboot_amd import engine, synth, trees
    letters, _ = synth.workload(shape)
    codes = synth.letters_to_codes(letters, "DNA")
    n, P = codes.shape
    eng = engine.FitchEngine(codes)
    back = trees.random_topology(n, np.random.default_rng(1))
    samples = np.random.default_rng(7).multinomial(P, np.ones(P) / P, size=n_samples).astype(np.uint16)
    eng.seed_ties(engine.TIE_RANDOM, 5)
    eng.score_tree(back)
    out = {"taxa": int(n), "columns": int(P), "kept_patterns": int(eng.num_informative), "row_words_padded": int(eng.Wp), "radius": radius,
           "samples": n_samples, "warm_ups": WARM, "calls_per_figure": REPS}
    out["plain_before"] = spread(timed(lambda: eng.tbr_sweep_best(radius)))

    def tracked(cutoff, timing):
        """WARM + REPS calls, each on a tracker attached afresh -> the figures of the timed ones"""
        wall, info, split = [], {}, {"k_tbr_masks": [], "product": [], "extraction": []}
        eng.set_option("timing", 1 if timing else 0)
        for k in range(WARM + REPS):
            eng.set_tree(back)
            eng.ufboot_attach(samples)
            if cutoff:
                eng.ufboot_set_cutoff(cutoff)
            ns0 = [eng.get_option(o) for o in ("tbr_masks_ns", "tbr_product_ns", "tbr_extract_ns")]
            t0 = time.perf_counter()
            _c, _f, _g, pairs = eng.ufboot_tbr_sweep(radius)
            ms = (time.perf_counter() - t0) * 1e3
            if k >= WARM:
                wall.append(ms)
                for key, o, z in zip(split, ("tbr_masks_ns", "tbr_product_ns", "tbr_extract_ns"), ns0):
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

    # the tracked SPR loop over one sweep's worth of prune-node visits, same tree, same radius
    def spr(cut):
        wall, booked = [], 0
        eng.set_option("max_visits", 2 * n - 2)
        for k in range(WARM + REPS):
            eng.set_tree(back)
            eng.seed_ties(engine.TIE_RANDOM, 5)
            eng.ufboot_attach(samples)
            if cut:
                eng.ufboot_set_cutoff(cut)
            t0 = time.perf_counter()
            eng.optimize_spr(1, radius)
            ms = (time.perf_counter() - t0) * 1e3
            if k >= WARM:
                wall.append(ms)
            booked = int(len(eng.ufboot_tree_logl()))
            eng.ufboot_detach()
        eng.set_option("max_visits", 0)
        return {"visits": 2 * n - 2, "booked": booked, "whole_call": spread(wall), "booked_per_s": booked / (statistics.median(wall) * 1e-3)}

    out["tracked_spr_no_cutoff"] = spr(0.0)
    out["tracked_spr_cutoff_top_10_percent"] = spr(cutoff)
    eng.set_tree(back)
    eng.score_tree(back)
    out["plain_after"] = spread(timed(lambda: eng.tbr_sweep_best(radius)))
    print(json.dumps(out))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("step %s ended with status %d: stopping here" % (" ".join(args), r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="C2", help="comma-separated: C2[,C3]")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=420, help="seconds a (shape, radius) step may take")
    ap.add_argument("--step", default=None)
    ap.add_argument("--radius", type=int, default=3)
    a = ap.parse_args()
    if a.step:
        step(a.step, a.radius, a.samples)
    else:
        res = {"protocol": "one MI355X, %d samples, %d warm-ups, median [min .. max] of %d whole calls" % (a.samples, WARM, REPS), "shapes": {}}
        for name in a.shapes.split(","):
            res["shapes"][name] = {}
            for rad in RADII:
                one = child(["--step", name, "--radius", str(rad), "--samples", str(a.samples)], a.limit)
                res["shapes"][name]["radius_%d" % rad] = one
                print(json.dumps({name: {rad: one}}), flush=True)
        if "C3" not in res["shapes"]:
            res["shapes"]["C3"] = "not timed"
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
