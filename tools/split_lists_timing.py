"""Time of the split products on trees with polytomies next to the host-only program, and of the record path next to a parent
build, DESIGN 5o.

    python tools/split_lists_timing.py --out profiles/split_lists/timing.json [--parent-root DIR]

(a) The new path.  The 5m shape (1000 trees x 1000 taxa, each 0 .. 16 local SPR moves from one tree, made as tools/splits_timing.py
    makes them), a random 0 .. 25 % of every tree's inner branches contracted, plus the greedy consensus of the set as one more
    tree.  Steps, each a child process of its own, every one that opens the GPU under `timeout`; a step that fails ends the run:

      lists   mpf_rf_distances_set, the whole call (wall clock), all pairs and "every tree against the consensus" (two sets), after a
              warm-up, `--reps` times: median, minimum and maximum.  Under the option "timing" the HIP-event time of the walk
              (split_keys_ns) for three calls of the same shape: the contracted trees as lists (k_split_keys_lists), the uncontracted
              trees as fully resolved lists (k_split_keys_lists) and as records (k_split_keys).
      host    mpboot_amd/host/split_lists_host_main.cpp built with -O2 and without a sanitizer, fed the same trees: ms_rf on one core,
              median of 3; its sum of distances must be the device's.

(b) No regression on the record path.  mpf_rf_distances and mpf_consensus_tree + mpf_split_support on record-format trees at the 5m /
    5n shape, this build and the one under --parent-root (a checkout of the parent commit with its library built: DIR/mpboot_amd) in
    five alternating rounds, each round a child process per build that imports that build's own package; the medians of this build
    against the minimum .. maximum of the parent's rounds.
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
if "--root" in sys.argv:                             # a child of part (b): the package of that build, not of this file's
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
else:
    sys.path.insert(0, ROOT)

TAXA, TREES, MOVES = 1000, 1000, 16


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def engine_for(n):
    from mpboot_amd import engine
    codes = (1 << np.random.default_rng(1).integers(0, 4, size=(n, 64))).astype(np.uint8)
    return engine.FitchEngine(codes)


def contract(backs, n, seed):
    """every tree with a random 0 .. 25 % of its inner branches contracted -> [(first, nbr)]"""
    from mpboot_amd import trees
    rng = np.random.default_rng(seed)
    out = []
    for b in backs:
        br = [(v, int(b[3 * v + s]) // 3) for v in range(n + 1, 2 * n - 1) for s in range(3) if int(b[3 * v + s]) // 3 > v]
        k = int(rng.integers(0, len(br) // 4 + 1))
        out.append(trees.collapse_branches(b, n, [br[int(i)] for i in rng.choice(len(br), size=k, replace=False)]))
    return out


def wall(call, reps):
    for _ in range(2):
        r = call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts), r


def keys_ms(e, call, reps):
    call()
    ts = []
    for _ in range(reps):
        k0 = e.get_option("split_keys_ns")
        call()
        ts.append((e.get_option("split_keys_ns") - k0) / 1e6)
    return spread(ts)


def step_lists(path, reps):
    from mpboot_amd import trees
    backs = np.load(path)
    n = TAXA
    e = engine_for(n)
    lists = contract(backs, n, 7)
    cons = e.consensus_tree(None, lists=lists)[:2]
    resolved = [trees.back_to_lists(b, n) for b in backs]
    everything = lists + [cons]
    out = {"inner_nodes": {"mean": float(np.mean([len(f) - 1 for f, _ in lists])), "consensus": len(cons[0]) - 1, "resolved": n - 2}}
    out["all_pairs_whole_call"], rf = wall(lambda: e.rf_distances(None, lists=everything), reps)
    out["rf_launches"], out["rf_columns"], out["overflow"] = (e.get_option(k) for k in ("rf_launches", "rf_columns", "split_overflow"))
    out["against_consensus_whole_call"], one = wall(lambda: e.rf_distances(None, None, lists=lists, lists2=[cons]), reps)
    assert (one[:, 0] == rf[:-1, -1]).all()
    out["sum"], out["mean_rf_to_consensus"] = int(rf.astype(np.int64).sum()), float(one.mean())
    e.set_option("timing", 1)
    out["split_keys"] = {"contracted_lists": keys_ms(e, lambda: e.rf_distances(None, lists=lists), reps),
                         "resolved_lists": keys_ms(e, lambda: e.rf_distances(None, lists=resolved), reps),
                         "records": keys_ms(e, lambda: e.rf_distances(backs), reps)}
    with open(path + ".sets", "wb") as f:
        np.array([n, 0, 0, 0, len(everything), 0, 0], dtype=np.int32).tofile(f)
        np.array([len(t[0]) - 1 for t in everything], dtype=np.int32).tofile(f)
        for k in (0, 1):
            for t in everything:
                np.asarray(t[k], dtype=np.int32).tofile(f)
    print(json.dumps(out))


def step_host(path, workdir):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(workdir, "split_lists_host")
    subprocess.check_call([cxx, "-std=c++17", "-O2", os.path.join(ROOT, "mpboot_amd", "host", "split_lists_host_main.cpp"), "-o", exe])
    ms, tail = [], {}
    for _ in range(3):
        r = subprocess.run([exe, "rf", path + ".sets", "quiet"], capture_output=True, text=True, check=True)
        tail = {ln.split()[0]: ln.split()[1] for ln in r.stdout.splitlines()}
        ms.append(float(tail["ms_rf"]))
    print(json.dumps({"ms_rf": spread(ms), "entries": int(tail["entries"]), "sum": int(tail["sum"]), "note": "one core, -O2"}))


def step_record(path, reps):
    """the record calls of 5m / 5n on the build whose package this process imported: medians of `reps` calls each"""
    backs = np.load(path)
    e = engine_for(TAXA)
    rf, _ = wall(lambda: e.rf_distances(backs), reps)

    def summary():
        e.consensus_tree(backs, None, 0.5)
        return e.split_support(backs, backs[0])

    sm, _ = wall(summary, reps)
    print(json.dumps({"rf_distances_ms": rf["median_ms"], "consensus_plus_support_ms": sm["median_ms"]}))


def child(args, limit=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    if limit:
        cmd = ["timeout", "-k", "10", str(limit)] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("step %s ended with status %d: stopping here" % (args[1], r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: adds part (b)")
    ap.add_argument("--step", default=None, choices=("lists", "host", "record"))
    ap.add_argument("--file", default=None)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--root", default=None)
    a = ap.parse_args()
    if a.step == "lists":
        step_lists(a.file, a.reps)
    elif a.step == "host":
        step_host(a.file, a.workdir)
    elif a.step == "record":
        step_record(a.file, a.reps)
    else:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from splits_timing import make_trees
        res = {"reps": a.reps, "shape": {"taxa": TAXA, "trees": TREES, "max_moves_per_tree": MOVES, "contracted": "0 .. 25 % of the inner branches"}}
        with tempfile.TemporaryDirectory() as wd:
            path = os.path.join(wd, "trees.npy")
            np.save(path, make_trees(TAXA, TREES, MOVES, 1))
            new = {"gpu": child(["--step", "lists", "--file", path, "--reps", str(a.reps)], limit=420)}
            new["host_program"] = child(["--step", "host", "--file", path, "--workdir", wd])
            new["same_sum_of_distances"] = new["gpu"]["sum"] == new["host_program"]["sum"]
            res["lists"] = new
            print(json.dumps({"lists": new}), flush=True)
            if a.parent_root:
                rounds = {"branch": [], "parent": []}
                for _ in range(a.rounds):
                    for who, root in (("parent", os.path.abspath(a.parent_root)), ("branch", ROOT)):
                        rounds[who].append(child(["--step", "record", "--file", path, "--reps", str(a.reps), "--root", root], limit=120))
                gate = {}
                for key in ("rf_distances_ms", "consensus_plus_support_ms"):
                    p = [r[key] for r in rounds["parent"]]
                    b = [r[key] for r in rounds["branch"]]
                    gate[key] = {"parent_rounds": p, "branch_rounds": b, "parent_median": statistics.median(p), "branch_median": statistics.median(b),
                                 "branch_median_within_parent_min_max": min(p) <= statistics.median(b) <= max(p),
                                 "branch_median_at_most_parent_max": statistics.median(b) <= max(p)}
                res["record_path"] = gate
                print(json.dumps({"record_path": gate}), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
