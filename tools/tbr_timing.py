"""Time of the TBR neighbourhood on the device, DESIGN 5q.

    python tools/tbr_timing.py --out profiles/tbr/timing.json

Synth C2 (200 x 10 000 DNA) and C3 (1000 x 50 000 DNA), a random tree each, radius 3 and radius 6.  Every step is a child process
of its own under `timeout`, one GPU process at a time; a step that fails ends the run.

  sweep  mpf_tbr_sweep_best: after 2 warm-up sweeps `--sweeps` (at least 20) sweeps, each timed as a whole call (wall clock) and, in
         a second pass under the option "timing", by HIP events around each chunk's three kernels (tbr_kernel_ns, summed over the
         sweep's chunks) -> pairs per second, chunks, the pair product's (pair x row word) rate
  yard   the same pairs as whole trees through mpf_score_trees (existing code): 64 drawn pairs, the time per tree extrapolated to
         all pairs of the sweep; and the (pair x row word) rate of k_place_costs in profiles/place/timing.json
  trace  rocprofv3 --kernel-trace --stats around 5 sweeps, a run of its own: the split between k_tbr_roots, k_tbr_costs and
         k_tbr_best
  climb  mpf_optimize_spr from one C2 start tree, then mpf_optimize_tbr from that SPR optimum: moves, lengths, wall clock
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("C2", "C3")
RADII = (3, 6)


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def setup(shape):
    from mpboot_amd import engine, synth, trees
    letters, _ = synth.workload(shape)
    codes = synth.letters_to_codes(letters, "DNA")
    eng = engine.FitchEngine(codes)
    back = trees.random_topology(codes.shape[0], np.random.default_rng(1))
    eng.score_tree(back)
    return eng, back, codes


def step_sweep(shape, radius, sweeps):
    from mpboot_amd import trees
    eng, back, codes = setup(shape)
    out = {"taxa": int(codes.shape[0]), "columns": int(codes.shape[1]), "kept_patterns": int(eng.num_informative), "row_words_padded": int(eng.Wp),
           "radius": radius}
    for _ in range(2):
        cost, f, g, pairs = eng.tbr_sweep_best(radius)
    wall = []
    for _ in range(sweeps):
        t0 = time.perf_counter()
        eng.tbr_sweep_best(radius)
        wall.append((time.perf_counter() - t0) * 1e3)
    eng.set_option("timing", 1)
    eng.tbr_sweep_best(radius)
    kern = []
    for _ in range(sweeps):
        k0 = eng.get_option("tbr_kernel_ns")
        eng.tbr_sweep_best(radius)
        kern.append((eng.get_option("tbr_kernel_ns") - k0) / 1e6)
    eng.set_option("timing", 0)
    out.update({"pairs": pairs, "chunks": eng.get_option("tbr_chunks"), "whole_call": spread(wall), "kernels": spread(kern),
                "pairs_per_s_whole_call": pairs / (statistics.median(wall) * 1e-3), "pairs_per_s_kernels": pairs / (statistics.median(kern) * 1e-3),
                "pair_words_per_s_kernels": pairs * eng.Wp / (statistics.median(kern) * 1e-3)})
    # yardstick: 64 drawn pairs as whole trees through mpf_score_trees
    rng = np.random.default_rng(2)
    order = eng.node_order().tolist()
    backs, want = [], []
    while len(backs) < 64:
        rec = order[int(rng.integers(len(order)))]
        ff, gg, m = eng.tbr_scan(rec, radius)
        if m.size <= 1:
            continue
        i, j = int(rng.integers(m.shape[0])), int(rng.integers(m.shape[1]))
        backs.append(trees.apply_tbr(back, rec, ([-1] + ff.tolist())[i], ([-1] + gg.tolist())[j]))
        want.append(int(m[i, j]))
    backs = np.stack(backs)
    eng.score_trees(backs)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = eng.score_trees(backs)
        ts.append((time.perf_counter() - t0) * 1e3)
    eng.score_tree(back)
    out["score_trees_route"] = {"trees": 64, "whole_call": spread(ts), "same_lengths": bool(got.tolist() == want),
                                "extrapolated_to_all_pairs_ms": statistics.median(ts) / 64 * pairs}
    out["speedup_over_score_trees_extrapolated"] = out["score_trees_route"]["extrapolated_to_all_pairs_ms"] / statistics.median(wall)
    print(json.dumps(out))


def step_trace(shape, radius):
    eng, _back, _codes = setup(shape)
    for _ in range(5):
        eng.tbr_sweep_best(radius)
    print(json.dumps({"sweeps": 5}))


def step_climb():
    eng, back, codes = setup("C2")
    t0 = time.perf_counter()
    spr = eng.optimize_spr(1, 6)
    t_spr = time.perf_counter() - t0
    t0 = time.perf_counter()
    tbr, moves = eng.optimize_tbr(6)
    t_tbr = time.perf_counter() - t0
    print(json.dumps({"shape": "C2", "radius": 6, "start_length": int(eng.score_tree(back)), "optimize_spr": {"length": spr, "seconds": t_spr},
                      "optimize_tbr_from_the_spr_optimum": {"length": tbr, "moves": moves, "seconds": t_tbr, "sweeps": moves + 1}}))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("step %s ended with status %d: stopping here" % (args[1], r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def traced(shape, radius, limit):
    """the kernels' shares of a run of its own under rocprofv3 --kernel-trace --stats (the program itself goes after --)"""
    with tempfile.TemporaryDirectory() as wd:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", wd, "--",
               sys.executable, os.path.abspath(__file__), "--step", "trace", "--shape", shape, "--radius", str(radius)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("the traced run ended with status %d: stopping here" % r.returncode)
        files = glob.glob(os.path.join(wd, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"note": "rocprofv3 wrote no kernel_stats.csv"}
        with open(files[0]) as f:
            rows = list(csv.DictReader(f))
    total = {}
    for row in rows:
        name = row.get("Name", "")
        ns = float(row.get("TotalDurationNs", 0) or 0)
        for k in ("k_tbr_roots", "k_tbr_costs", "k_tbr_best"):
            if k in name:
                total[k] = total.get(k, 0.0) + ns
    s = sum(total.values())
    return {"sweeps": 5, "ns": total, "share": {k: v / s for k, v in total.items()} if s else {}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=SHAPES)
    ap.add_argument("--radius", type=int, default=6)
    ap.add_argument("--step", default=None, choices=("sweep", "trace", "climb"))
    a = ap.parse_args()
    if a.step == "sweep":
        step_sweep(a.shape, a.radius, max(20, a.sweeps))
    elif a.step == "trace":
        step_trace(a.shape, a.radius)
    elif a.step == "climb":
        step_climb()
    else:
        res = {"sweeps_per_figure": max(20, a.sweeps), "shapes": {}}
        with open(os.path.join(ROOT, "profiles", "place", "timing.json")) as f:
            pl = json.load(f)["shapes"]["C3"]["query_sweep"]["k_place_costs_rate"]
        res["k_place_costs_yardstick"] = {"operations_per_s": pl["operations_per_s"], "from": "profiles/place/timing.json, C3, wide shape"}
        for name in SHAPES:
            if a.shape and a.shape != name:
                continue
            res["shapes"][name] = {}
            for rad in RADII:
                one = child(["--step", "sweep", "--shape", name, "--radius", str(rad), "--sweeps", str(a.sweeps)], limit=420)
                one["kernel_split"] = traced(name, rad, 300)
                share = one["kernel_split"].get("share", {}).get("k_tbr_costs")
                if share:
                    one["k_tbr_costs_pair_words_per_s"] = one["pairs"] * one["row_words_padded"] / (one["kernels"]["median_ms"] * 1e-3 * share)
                    one["k_tbr_costs_over_k_place_costs_rate"] = one["k_tbr_costs_pair_words_per_s"] / pl["operations_per_s"]
                res["shapes"][name]["radius_%d" % rad] = one
                print(json.dumps({name: {rad: one}}), flush=True)
        res["climb"] = child(["--step", "climb"], limit=600)
        print(json.dumps(res["climb"]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
