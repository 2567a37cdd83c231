"""Time of the TBR neighbourhood on the weighted (-cost) engine next to the only route there was before, DESIGN 5q (weighted section).

    python tools/tbr_snk_timing.py --out profiles/tbr/timing_weighted.json [--with-c3]

Workloads: synth C2 (200 x 10 000 DNA) under the transition / transversion matrix at radius 3 and 6, each in the 16-bit store and
in the 32-bit store (option "sankoff_short"); C5 (500 x 20 000 protein) under a 20 x 20 metric at radius 3; with --with-c3 also C3
(1000 x 50 000 DNA) under tstv at radius 3.  A random tree each.  Every workload is a child process of its own under `timeout`, one
GPU process at a time; a step that fails ends the run.

  sweep  mpf_tbr_sweep_best under "tbr_weighted": after 2 warm-up sweeps `--sweeps` (at least 7) sweeps, each timed as a whole call
         (wall clock) and, in a second pass under the option "timing", by HIP events around each chunk's three kernels
         (tbr_kernel_ns, summed over the sweep's chunks) -> pairs per second, chunks.  tbr_tile left free (0) and forced narrow (1)
         and wide (2)
  yard   the same pairs as whole trees through mpf_score_trees (existing code, the route a user had): 64 drawn pairs, the time per
         tree EXTRAPOLATED to all pairs of the sweep and marked so.  The drawn entries must equal the scan's
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

# (workload, matrix, alphabet, radius, stores)
STEPS = [("C2", "tstv", "DNA", 3, (1, 0)), ("C2", "tstv", "DNA", 6, (1, 0)), ("C5", "metric20", "AA", 3, (1,))]
C3_STEP = ("C3", "tstv", "DNA", 3, (1,))
TILES = {0: "rule", 1: "narrow", 2: "wide"}


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


def step_sweep(shape, kind, alphabet, radius, short, sweeps):
    from mpboot_amd import engine, synth, trees
    letters, _ = synth.workload(shape)
    codes = synth.letters_to_codes(letters, alphabet)
    eng = engine.FitchEngine(codes, datatype=0 if alphabet == "DNA" else 1, cost=matrix(kind))
    eng.set_option("tbr_weighted", 1)
    eng.set_option("sankoff_short", short)
    back = trees.random_topology(codes.shape[0], np.random.default_rng(1))
    length = eng.score_tree(back)
    out = {"taxa": int(codes.shape[0]), "columns": int(codes.shape[1]), "kept_patterns": int(eng.num_informative), "row_patterns_padded": int(eng.Wp),
           "matrix": kind, "radius": radius, "store_bits": 16 if eng.get_option("sankoff_packed") else 32, "length": int(length), "tiles": {}}
    bests = None
    for tile, name in TILES.items():
        eng.set_option("tbr_tile", tile)
        for _ in range(2):
            cost, f, g, pairs = eng.tbr_sweep_best(radius)
        got = (cost.tolist(), f.tolist(), g.tolist())
        assert bests is None or got == bests, "the shapes disagree"
        bests = got
        wall = []
        for _ in range(sweeps):
            t0 = time.perf_counter()
            eng.tbr_sweep_best(radius)
            wall.append((time.perf_counter() - t0) * 1e3)
        eng.set_option("timing", 1)
        eng.tbr_sweep_best(radius)
        kern, l0 = [], eng.get_option("tbr_launches")
        for _ in range(sweeps):
            k0 = eng.get_option("tbr_kernel_ns")
            eng.tbr_sweep_best(radius)
            kern.append((eng.get_option("tbr_kernel_ns") - k0) / 1e6)
        eng.set_option("timing", 0)
        out["tiles"][name] = {"whole_call": spread(wall), "kernels": spread(kern), "cost_launches_per_sweep": (eng.get_option("tbr_launches") - l0) / sweeps,
                              "pairs_per_s_whole_call": pairs / (statistics.median(wall) * 1e-3),
                              "pairs_per_s_kernels": pairs / (statistics.median(kern) * 1e-3)}
    eng.set_option("tbr_tile", 0)
    out.update({"pairs": pairs, "chunks": eng.get_option("tbr_chunks")})
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
    rule = out["tiles"]["rule"]["whole_call"]["median_ms"]
    out["score_trees_route"] = {"trees": 64, "whole_call": spread(ts), "same_lengths": bool(got.tolist() == want),
                                "extrapolated_to_all_pairs_ms": statistics.median(ts) / 64 * pairs, "extrapolated": True}
    out["speedup_over_score_trees_extrapolated"] = out["score_trees_route"]["extrapolated_to_all_pairs_ms"] / rule
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
    ap.add_argument("--sweeps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--with-c3", action="store_true")
    ap.add_argument("--step", default=None, help="internal: shape,matrix,alphabet,radius,short")
    a = ap.parse_args()
    if a.step:
        shape, kind, alphabet, radius, short = a.step.split(",")
        step_sweep(shape, kind, alphabet, int(radius), int(short), max(7, a.sweeps))
    else:
        res = {"sweeps_per_figure": max(7, a.sweeps), "workloads": {}}
        for shape, kind, alphabet, radius, stores in STEPS + ([C3_STEP] if a.with_c3 else []):
            for short in stores:
                one = child(["--step", "%s,%s,%s,%d,%d" % (shape, kind, alphabet, radius, short), "--sweeps", str(a.sweeps)], limit=400)
                res["workloads"]["%s_%s_radius_%d_%d_bit" % (shape, kind, radius, one["store_bits"])] = one
                print(json.dumps({shape: {radius: one}}), flush=True)
                if a.out:                                    # (after every workload: a run that is cut short leaves what it had)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump(res, f, indent=1)
                        f.write("\n")
