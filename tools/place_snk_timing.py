"""Time of taxon insertion on the weighted (-cost) engine next to the only route there was before, DESIGN 5p (weighted section).

    python tools/place_snk_timing.py --out profiles/place/timing_weighted.json

Inputs: synth C2 (200 x 10 000 DNA) and C3 (1000 x 50 000 DNA) under the transition / transversion matrix, C5 (500 x 20 000
protein) under a 20 x 20 metric, and AA1200 (1200 x 1000 protein, 768 held out: the crossing of the two shapes on 20 rows); a random
tree each.  Each input in the 16-bit store and in the 32-bit store (option
"sankoff_short").  Every input is a child process of its own under `timeout`, one GPU process at a time; a step that fails ends the
run.

  new    mpf_insertion_costs under "place_weighted": ONE query (the last taxon) on the (n - 1)-tip backbone, and Q = 16, 64, 256
         queries on a backbone with 256 taxa held out (C2: 100, and no Q = 256).  Whole call (wall clock) and, in a
         second pass under the option "timing", place_kernel_ns and poly_view_ns per call: median, minimum, maximum of `--reps`
         after two warm-ups.  place_tile left free (0) and forced narrow (1) and wide (2).
  route  the same numbers through mpf_compute_parsimony_at over the completed trees, root_taxon = the query: every tree of the
         one-query case where there are at most `--route-trees` of them, otherwise that many trees drawn at random, the whole
         matrix's time EXTRAPOLATED as trees x median time per tree and marked so.  The sampled entries must equal the new path's.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INPUTS = {"C2": "tstv", "C3": "tstv", "C5": "metric20", "AA1200": "metric20s"}
# AA1200: 1200 x 1000 protein under a 20 x 20 metric with small entries (the 16-bit store takes 1200 taxa), 768 taxa held out: enough
# outputs (Q = 256, 512, 768 on 861 branches) to find where the two shapes cross on 20 rows; the crossing is a number of outputs,
# both shapes' times growing with the row length alike
EXTRA = {"AA1200": dict(n_taxa=1200, n_patterns=1000, alphabet="AA", r=0.08, seed=21, held=768, queries=(256, 512, 768))}


def matrix(kind):
    if kind == "tstv":
        c = np.full((4, 4), 2, dtype=np.uint32)
        np.fill_diagonal(c, 0)
        c[0, 2] = c[2, 0] = c[1, 3] = c[3, 1] = 1
        return c
    pts = np.random.default_rng(4).integers(0, 4 if kind == "metric20s" else 12, size=(20, 3))     # Manhattan distances of random points: symmetric, closed
    c = np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2).astype(np.uint32)
    c[c == 0] = 1
    np.fill_diagonal(c, 0)
    return c


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def timed(eng, call, reps):
    for _ in range(2):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    eng.set_option("timing", 1)
    for _ in range(2):
        call()
    kern, view = [], []
    for _ in range(reps):
        k0, v0 = eng.get_option("place_kernel_ns"), eng.get_option("poly_view_ns")
        call()
        kern.append((eng.get_option("place_kernel_ns") - k0) / 1e6)
        view.append((eng.get_option("poly_view_ns") - v0) / 1e6)
    eng.set_option("timing", 0)
    return {"whole_call": spread(wall), "place_kernels": spread(kern), "k_poly_snk_views": spread(view)}


def tiles(eng, call, reps):
    r = timed(eng, call, reps)
    for tile, name in ((1, "narrow"), (2, "wide")):
        eng.set_option("place_tile", tile)
        f = timed(eng, call, reps)
        r["whole_call_" + name], r["place_kernels_" + name] = f["whole_call"], f["place_kernels"]
    eng.set_option("place_tile", 0)
    return r


def step_gpu(shape, reps, route_trees):
    from mpboot_amd import engine, synth, trees
    cfg = synth.WORKLOADS.get(shape) or EXTRA[shape]
    letters, _ = synth.synth_alignment(cfg["n_taxa"], cfg["n_patterns"], cfg["alphabet"], cfg["r"], cfg["seed"])
    codes = synth.letters_to_codes(letters, cfg["alphabet"])
    n = codes.shape[0]
    eng = engine.FitchEngine(codes, datatype=engine.DNA if cfg["alphabet"] == "DNA" else engine.AA, cost=matrix(INPUTS[shape]))
    eng.set_option("place_weighted", 1)
    lib = engine.load_library()
    rng = np.random.default_rng(1)
    back = trees.random_topology(n, rng)
    first, nbr = trees.drop_tips(back, n, [n])
    held = cfg.get("held", 256 if n >= 500 else n // 2)       # (C2 has no 256 to hold out beside a backbone)
    drop = (rng.permutation(n - 1)[:held] + 2).tolist()                 # (tip 1 stays: the root leaf)
    f2, n2 = trees.drop_tips(back, n, drop)
    out = {"taxa": n, "columns": int(codes.shape[1]), "kept_patterns": int(eng.num_informative), "matrix": INPUTS[shape], "stores": {}}

    def at(b, root):
        s = C.c_uint32()
        b = np.ascontiguousarray(b, dtype=np.int32)
        if lib.mpf_compute_parsimony_at(eng.h, b.ctypes.data_as(C.c_void_p), root, C.byref(s), None):
            raise SystemExit("mpf_compute_parsimony_at failed")
        return int(s.value)

    for short in (1, 0):
        eng.set_option("sankoff_short", short)
        st = {"sankoff_packed": int(eng.get_option("sankoff_packed"))}
        a, b, cost, _ = eng.insertion_costs(first, nbr, [n])
        one = tiles(eng, lambda: eng.insertion_costs(first, nbr, [n]), reps)
        one["branches"] = len(a)
        # the route of the parent commit: the completed trees one by one
        pick = list(range(len(a))) if len(a) <= route_trees else sorted(rng.permutation(len(a))[:route_trees].tolist())
        backs = [trees.lists_to_back(*trees.insert_tip(first, nbr, n, n, int(a[i]), int(b[i])), n) for i in pick]
        same = all(at(bk, n) == int(cost[0, i]) for bk, i in zip(backs, pick))        # (the warm-up)
        per_tree = []
        for _ in range(3):
            t0 = time.perf_counter()
            for bk in backs:
                at(bk, n)
            per_tree.append((time.perf_counter() - t0) * 1e3 / len(backs))
        ms = statistics.median(per_tree)
        one["compute_parsimony_at_route"] = {"trees_timed": len(backs), "per_tree": spread(per_tree), "same_entries": bool(same),
                                             "whole_matrix_ms": ms * len(a), "extrapolated": len(backs) < len(a)}
        one["speedup_over_the_route"] = ms * len(a) / one["whole_call"]["median_ms"]
        st["one_query"] = one
        sweep = {"held_out": held, "backbone_tips": n - held, "branches": 2 * (n - held) - 3, "queries": {}}
        for Q in cfg.get("queries", (16, 64, 256)):
            if Q > held:
                continue
            r = tiles(eng, lambda: eng.insertion_costs(f2, n2, drop[:Q]), reps)
            pt, _, _, ln, _ = eng.place_taxa(f2, n2, drop[:Q])
            full = eng.insertion_costs(f2, n2, drop[:Q])[2]
            r["place_taxa_is_the_first_minimum"] = bool((pt == full.argmin(axis=1)).all() and (ln == full.min(axis=1)).all())
            # the route: Q x branches completed trees of n - held + 1 tips are no trees mpf_compute_parsimony_at takes (it wants every
            # taxon); its time per tree on this input is the one measured above, on the larger (n-tip) trees
            r["compute_parsimony_at_route"] = {"whole_matrix_ms": ms * Q * sweep["branches"], "extrapolated": True,
                                               "note": "per-tree time of the one-query case (n-tip trees) x Q x branches"}
            sweep["queries"][str(Q)] = r
        st["query_sweep"] = sweep
        out["stores"]["16-bit" if short else "32-bit"] = st
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--route-trees", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=tuple(INPUTS), help="one input only")
    ap.add_argument("--step", default=None, choices=("gpu",))
    a = ap.parse_args()
    if a.step == "gpu":
        step_gpu(a.shape, a.reps, a.route_trees)
    else:
        res = {"reps": a.reps, "inputs": {}}
        ok = True
        for name in INPUTS:
            if a.shape and a.shape != name:
                continue
            one = child(["--step", "gpu", "--shape", name, "--reps", str(a.reps), "--route-trees", str(a.route_trees)], limit=400)
            ok = ok and all(s["one_query"]["compute_parsimony_at_route"]["same_entries"] for s in one["stores"].values())
            res["inputs"][name] = one
            print(json.dumps({name: one}), flush=True)
            if a.out:                                           # (written after every input: a later step's failure loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
        if not ok:
            raise SystemExit("the entries differ between the new path and mpf_compute_parsimony_at")
