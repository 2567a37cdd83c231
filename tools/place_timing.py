"""Time of taxon insertion on the device next to the two other routes to the same numbers, DESIGN 5p.

    python tools/place_timing.py --out profiles/place/timing.json

Two shapes, synth C2 (200 x 10 000 DNA) and C3 (1000 x 50 000 DNA), a random tree each.  Steps, each a child process of its own,
every one that opens the GPU under `timeout`, one GPU process at a time; a step that fails ends the run:

  gpu    1. mpf_insertion_costs of ONE query (the last taxon) on the (n - 1)-tip backbone: the whole call (wall clock, after a
            warm-up, `--reps` times: median, minimum, maximum) and, in a second run under the option "timing", place_kernel_ns and
            poly_view_ns per call.
         2. the same 2 n - 5 numbers by the only route there was before: mpf_score_trees over the completed trees (existing code).
         4. Q = 1, 16, 64, 256 queries on a backbone with min(256, n / 2) taxa held out (C2 has no 256 to hold out beside a
            backbone): whole call and kernel time; mpf_place_taxa of the same queries, kernel time (k_place_costs + k_place_best).
         5. for the kernel at the largest Q the (query, branch, word) operations per second it achieved -- tiles x tile area x
            padded words -- next to the VALU issue bound, computed as tools/rf_timing.py computes its own: 256 CUs x 4 SIMDs x 32
            lanes per cycle x 2.4 GHz / 5 instructions per operation (four v_and / v_and_or and one v_bcnt for 4 state rows).
  host   3. mpboot_amd/host/place_host_main.cpp built with -O2 and without a sanitizer, fed the engine's own tip vectors and the
            same backbone: its host_costs on one core, median of 3.
The costs of 1, 2 and 3 must be equal, and 1 must be faster than 2; the run fails otherwise.

    python tools/place_timing.py --compare-lib OTHER/libmpfitch.so --out profiles/place/timing_list_tree.json

Two builds of the library next to each other -- this tree's and another commit's -- on the host-bound calls: the one-query call
of step 1 and mpf_iq_parsimony_tree (n - 3 such steps with the host's check, plan and list growth between them), both shapes.  Each
build runs in child processes of its own (MPF_LIB_PATH), `--rounds` of them per shape, the two builds taking turns; a round's
figure is its median, a build's figure the median of its rounds and its spread their maximum minus their minimum.  Accepted: the same
costs and the same tree from both, and this build's figure not above the other's by more than the larger of the two spreads.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("C2", "C3")
VALU_OP_BOUND = 256 * 4 * 32 * 2.4e9 / 5
WIDE_DNA = (64, 64)


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def timed(eng, call, reps):
    """whole-call wall clock and, in a second pass under "timing", the kernels' HIP-event time per call"""
    for _ in range(2):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    eng.set_option("timing", 1)
    call()
    kern, view = [], []
    for _ in range(reps):
        k0, v0 = eng.get_option("place_kernel_ns"), eng.get_option("poly_view_ns")
        call()
        kern.append((eng.get_option("place_kernel_ns") - k0) / 1e6)
        view.append((eng.get_option("poly_view_ns") - v0) / 1e6)
    eng.set_option("timing", 0)
    return {"whole_call": spread(wall), "place_kernels": spread(kern), "k_poly_views": spread(view)}


def step_gpu(shape, reps, workdir):
    from mpboot_amd import engine, synth, trees
    letters, _ = synth.workload(shape)
    codes = synth.letters_to_codes(letters, "DNA")
    n = codes.shape[0]
    eng = engine.FitchEngine(codes)
    rng = np.random.default_rng(1)
    back = trees.random_topology(n, rng)
    first, nbr = trees.drop_tips(back, n, [n])
    out = {"taxa": n, "columns": int(codes.shape[1]), "kept_patterns": int(eng.num_informative), "row_words_padded": int(eng.Wp)}
    # 1: one query on the (n - 1)-tip backbone
    a, b, cost, length = eng.insertion_costs(first, nbr, [n])
    one = timed(eng, lambda: eng.insertion_costs(first, nbr, [n]), reps)
    one["branches"] = len(a)
    out["one_query"] = one
    # 2: the completed trees through mpf_score_trees
    backs = np.stack([trees.lists_to_back(*trees.insert_tip(first, nbr, n, n, int(a[i]), int(b[i])), n) for i in range(len(a))])
    scores = eng.score_trees(backs)
    wall = []
    for _ in range(max(3, reps // 2)):
        t0 = time.perf_counter()
        scores = eng.score_trees(backs)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["score_trees_route"] = {"whole_call": spread(wall), "trees": len(backs)}
    out["same_costs_as_score_trees"] = bool((scores.astype(np.int64) == cost[0].astype(np.int64)).all())
    out["one_query_speedup_over_score_trees"] = statistics.median(wall) / one["whole_call"]["median_ms"]
    # the host program's input: the engine's own tip vectors
    np.save(os.path.join(workdir, shape + "_row.npy"), cost[0].astype(np.int64))
    with open(os.path.join(workdir, shape + ".bin"), "wb") as f:
        np.array([n, eng.S, eng.W, len(first) - 1, 1, 1], dtype=np.int32).tofile(f)
        first.tofile(f)
        nbr.tofile(f)
        np.array([n], dtype=np.int32).tofile(f)
        for t in range(1, n + 1):
            eng.tip_vector(t).tofile(f)
    # 4, 5: the query sweep
    held = min(256, n // 2)
    drop = (rng.permutation(n - 1)[:held] + 2).tolist()                 # (tip 1 stays: the root leaf)
    f2, n2 = trees.drop_tips(back, n, drop)
    sweep = {"held_out": held, "backbone_tips": n - held, "branches": 2 * (n - held) - 3, "queries": {}}
    for Q in (1, 16, 64, 256):
        if Q > held:
            continue
        r = timed(eng, lambda: eng.insertion_costs(f2, n2, drop[:Q]), reps)
        for tile, name in ((1, "narrow"), (2, "wide")):            # the two shapes forced, kernel time only
            eng.set_option("place_tile", tile)
            r["place_kernels_" + name] = timed(eng, lambda: eng.insertion_costs(f2, n2, drop[:Q]), reps)["place_kernels"]
        eng.set_option("place_tile", 0)
        at, _, _, ln, _ = eng.place_taxa(f2, n2, drop[:Q])
        r["place_taxa_kernels"] = timed(eng, lambda: eng.place_taxa(f2, n2, drop[:Q]), reps)["place_kernels"]      # (k_place_best rides in it)
        full = eng.insertion_costs(f2, n2, drop[:Q])[2]
        r["place_taxa_is_the_first_minimum"] = bool((at == full.argmin(axis=1)).all() and (ln == full.min(axis=1)).all())
        sweep["queries"][str(Q)] = r
        last = (Q, r)
    Q, r = last
    tq, tb = WIDE_DNA
    tiles = -(-Q // tq) * -(-sweep["branches"] // tb)
    ops = tiles * tq * tb * eng.Wp
    rate = ops / (r["place_kernels_wide"]["median_ms"] * 1e-3)
    sweep["k_place_costs_rate"] = {"queries": Q, "tiles": tiles, "padded_words_per_row": int(eng.Wp), "operations": ops, "operations_per_s": rate,
                                   "useful_fraction_of_the_tiles": Q * sweep["branches"] / (tiles * tq * tb),
                                   "valu_issue_bound_operations_per_s": VALU_OP_BOUND, "fraction_of_bound": rate / VALU_OP_BOUND}
    out["query_sweep"] = sweep
    print(json.dumps(out))


def step_ab(shape, reps):
    """one round of one build: wall clock of the one-query call and of mpf_iq_parsimony_tree, and what they returned"""
    import hashlib

    from mpboot_amd import engine, synth, trees
    letters, _ = synth.workload(shape)
    codes = synth.letters_to_codes(letters, "DNA")
    n = codes.shape[0]
    eng = engine.FitchEngine(codes)
    first, nbr = trees.drop_tips(trees.random_topology(n, np.random.default_rng(1)), n, [n])
    order = np.arange(1, n + 1)
    cost = eng.insertion_costs(first, nbr, [n])[2]
    tree = eng.iq_parsimony_tree(order=order)
    one, grow = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.insertion_costs(first, nbr, [n])
        one.append((time.perf_counter() - t0) * 1e3)
    for _ in range(3):
        t0 = time.perf_counter()
        eng.iq_parsimony_tree(order=order)
        grow.append((time.perf_counter() - t0) * 1e3)
    h = hashlib.sha256()
    for a in (cost, tree[0], tree[1], tree[2]):
        h.update(np.ascontiguousarray(a).tobytes())
    print(json.dumps({"taxa": n, "library": engine.LIB_PATH, "one_query_ms": statistics.median(one), "iq_parsimony_tree_ms": statistics.median(grow),
                      "results_sha256": h.hexdigest()}))


def compare(other_lib, shapes, reps, rounds):
    res = {"reps": reps, "rounds": rounds, "shapes": {}}
    ok = True
    for name in shapes:
        got = {"other": [], "this": []}
        for _ in range(rounds):
            for side in ("other", "this"):
                env = dict(os.environ)
                if side == "other":
                    env["MPF_LIB_PATH"] = os.path.abspath(other_lib)
                else:
                    env.pop("MPF_LIB_PATH", None)
                got[side].append(child(["--step", "ab", "--shape", name, "--reps", str(reps)], limit=300, env=env))
        one = {"taxa": got["this"][0]["taxa"]}
        one["same_results"] = len({r["results_sha256"] for side in got.values() for r in side}) == 1
        ok = ok and one["same_results"]
        for what in ("one_query_ms", "iq_parsimony_tree_ms"):
            fig = {}
            for side in got:
                xs = [r[what] for r in got[side]]
                fig[side] = {"median_ms": statistics.median(xs), "spread_ms": max(xs) - min(xs), "rounds_ms": xs}
            fig["accepted"] = fig["this"]["median_ms"] <= fig["other"]["median_ms"] + max(fig["this"]["spread_ms"], fig["other"]["spread_ms"])
            ok = ok and fig["accepted"]
            one[what] = fig
        res["shapes"][name] = one
        print(json.dumps({name: one}), flush=True)
    res["accepted"] = ok
    return res


def step_host(shape, workdir):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(workdir, "place_host")
    if not os.path.exists(exe):
        subprocess.check_call([cxx, "-std=c++17", "-O2", os.path.join(ROOT, "mpboot_amd", "host", "place_host_main.cpp"), "-o", exe])
    want = np.load(os.path.join(workdir, shape + "_row.npy")).tolist()
    ms, same = [], True
    for _ in range(3):
        r = subprocess.run([exe, "costs", os.path.join(workdir, shape + ".bin")], capture_output=True, text=True, check=True)
        lines = r.stdout.splitlines()
        row = next([int(x) for x in ln.split()[2:]] for ln in lines if ln.startswith("row 0"))
        same = same and row == want
        ms.append(float(next(ln for ln in lines if ln.startswith("seconds")).split()[1]) * 1e3)
    print(json.dumps({"host_costs": spread(ms), "same_costs_as_the_engine": same, "note": "one core, -O2, views and costs"}))


def child(args, limit=None, env=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    if limit:
        cmd = ["timeout", "-k", "10", str(limit)] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("step %s ended with status %d: stopping here" % (args[1], r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=SHAPES, help="one shape only")
    ap.add_argument("--step", default=None, choices=("gpu", "host", "ab"))
    ap.add_argument("--compare-lib", default=None, help="another commit's libmpfitch.so: time the host-bound calls of both builds in turn")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    if a.step == "gpu":
        step_gpu(a.shape, a.reps, a.workdir)
    elif a.step == "host":
        step_host(a.shape, a.workdir)
    elif a.step == "ab":
        step_ab(a.shape, a.reps)
    elif a.compare_lib:
        res = compare(a.compare_lib, [a.shape] if a.shape else SHAPES, a.reps, a.rounds)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        if not res["accepted"]:
            raise SystemExit("the two builds differ in their results, or this one is slower than the other by more than the spread")
    else:
        res = {"reps": a.reps, "shapes": {}}
        ok = True
        with tempfile.TemporaryDirectory() as wd:
            for name in SHAPES:
                if a.shape and a.shape != name:
                    continue
                one = child(["--step", "gpu", "--shape", name, "--reps", str(a.reps), "--workdir", wd], limit=420)
                one["host_program"] = child(["--step", "host", "--shape", name, "--workdir", wd])
                one["host_over_one_query_call"] = one["host_program"]["host_costs"]["median_ms"] / one["one_query"]["whole_call"]["median_ms"]
                ok = ok and one["same_costs_as_score_trees"] and one["host_program"]["same_costs_as_the_engine"] and \
                    one["one_query_speedup_over_score_trees"] > 1.0
                res["shapes"][name] = one
                print(json.dumps({name: one}), flush=True)
        res["accepted"] = ok
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        if not ok:
            raise SystemExit("the costs differ between the routes, or the one-query call is not faster than mpf_score_trees")
