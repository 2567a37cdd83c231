"""Time of the bootstrap summary on the device next to two CPU yardsticks, DESIGN 5m.

    python tools/splits_timing.py --out profiles/splits/timing.json          # 1000 trees x 1000 taxa

The tree set: one random topology of `--taxa` taxa and `--trees` copies of it, each 0 .. `--moves` local SPR moves away (prune a
subtree, regraft it at most six branches off: what the trees of a bootstrap run look like next to each other).  Steps, each a child
process of its own, every one that opens the GPU under `timeout`; a step that fails ends the run:

  gpu      mpf_consensus_tree + mpf_split_support (the whole calls, wall clock, and the HIP-event time of the kernels inside them:
           read-only options split_keys_ns / split_count_ns / split_bits_ns under "timing"), and mpf_split_counts alone
  host     mpboot_amd/host/splits_host_main.cpp built with -O2 and without a sanitizer, fed the same trees: the host's own exact
           count, supports, order and consensus -- the honest CPU comparison
  witness  collections.Counter over trees.splits on 20 of the trees, scaled to the whole set and labelled as scaled
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpboot_amd import trees  # noqa: E402


def local_spr(b, n, rng, radius=6):
    """one SPR move: prune at record p of an inner node, regraft 1 .. radius branches away from where it hung"""
    while True:
        v = int(rng.integers(n + 1, 2 * n - 1))
        p = 3 * v + int(rng.integers(0, 3))
        ends = [int(b[trees.nxt(p)]), int(b[trees.nxt(trees.nxt(p))])]
        r = ends[int(rng.integers(0, 2))]
        if r // 3 <= n:
            continue
        for _ in range(int(rng.integers(1, radius + 1))):
            if r // 3 <= n:
                break
            r = int(b[trees.nxt(r) if rng.integers(0, 2) else trees.nxt(trees.nxt(r))])
        return trees.apply_spr(b, p, int(b[r]))


def make_trees(n, T, moves, seed):
    rng = np.random.default_rng(seed)
    base = trees.random_topology(n, rng)
    out = np.empty((T, len(base)), dtype=np.int32)
    for t in range(T):
        b = base
        for _ in range(int(rng.integers(0, moves + 1))):
            b = local_spr(b, n, rng)
        out[t] = b
    trees.validate(out[T - 1], n)
    return out


def load(path):
    with open(path, "rb") as f:
        n, T, _hw = np.fromfile(f, dtype=np.int32, count=3)
        return int(n), np.fromfile(f, dtype=np.int32).reshape(int(T), -1)


def step_gpu(path, reps):
    from mpboot_amd import engine
    n, backs = load(path)
    codes = (1 << np.random.default_rng(1).integers(0, 4, size=(n, 64))).astype(np.uint8)
    e = engine.FitchEngine(codes)
    e.set_option("timing", 1)
    target = backs[0]
    out = {}
    for name, thr in (("majority", 0.5), ("greedy", 0.0)):
        for _ in range(2):
            e.consensus_tree(backs, None, thr)
            e.split_support(backs, target)
        k0 = [e.get_option(k) for k in ("split_keys_ns", "split_count_ns", "split_bits_ns")]
        t0 = time.perf_counter()
        for _ in range(reps):
            first, nbr, sup, total = e.consensus_tree(backs, None, thr)
            e.split_support(backs, target)
        wall = (time.perf_counter() - t0) / reps
        k1 = [e.get_option(k) for k in ("split_keys_ns", "split_count_ns", "split_bits_ns")]
        out[name] = {"threshold": thr, "whole_calls_ms": wall * 1e3, "inner_nodes": len(first) - 1,
                     "kernels_ms": {"k_split_keys": (k1[0] - k0[0]) / reps / 1e6, "insert_count_compact_gather": (k1[1] - k0[1]) / reps / 1e6,
                                    "k_split_bits": (k1[2] - k0[2]) / reps / 1e6},
                     "note": "two passes over the trees per repetition: one for the consensus, one for the supports"}
    e.split_counts(backs)
    t0 = time.perf_counter()
    for _ in range(reps):
        bits, count, total = e.split_counts(backs)
    out["split_counts"] = {"whole_call_ms": (time.perf_counter() - t0) / reps * 1e3, "distinct": len(count), "total_weight": total,
                           "overflow": e.get_option("split_overflow")}
    print(json.dumps(out))


def step_host(path, workdir):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(workdir, "splits_host")
    subprocess.check_call([cxx, "-std=c++17", "-O2", os.path.join(ROOT, "mpboot_amd", "host", "splits_host_main.cpp"), "-o", exe])
    out = {}
    for name, thr in (("majority", 0.5), ("greedy", 0.0)):
        r = subprocess.run([exe, "trees", path, str(thr), "quiet"], capture_output=True, text=True, check=True)
        ms = {ln.split()[0]: float(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("ms_")}
        ms["whole_ms"] = sum(ms.values())
        ms["distinct"] = int(next(ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("n_distinct")))
        out[name] = ms
    print(json.dumps(out))


def step_witness(path, sample):
    from collections import Counter
    n, backs = load(path)
    t0 = time.perf_counter()
    c = Counter()
    for b in backs[:sample]:
        for s in trees.splits(b):
            c[s] += 1
    dt = time.perf_counter() - t0
    print(json.dumps({"trees_timed": sample, "seconds_timed": dt, "scaled_to_all_trees_s": dt * len(backs) / sample,
                      "note": "scaled from %d trees; the count only, no order, no consensus" % sample}))


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
    ap.add_argument("--taxa", type=int, default=1000)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--moves", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=("gpu", "host", "witness"))
    ap.add_argument("--file", default=None)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    if a.step == "gpu":
        step_gpu(a.file, a.reps)
    elif a.step == "host":
        step_host(a.file, a.workdir)
    elif a.step == "witness":
        step_witness(a.file, 20)
    else:
        with tempfile.TemporaryDirectory() as wd:
            path = os.path.join(wd, "trees.bin")
            backs = make_trees(a.taxa, a.trees, a.moves, 1)
            with open(path, "wb") as f:
                np.array([a.taxa, a.trees, 0], dtype=np.int32).tofile(f)
                backs.tofile(f)
            res = {"taxa": a.taxa, "trees": a.trees, "max_moves_per_tree": a.moves, "reps": a.reps}
            res["gpu"] = child(["--step", "gpu", "--file", path, "--reps", str(a.reps)], limit=300)
            res["host_program"] = child(["--step", "host", "--file", path, "--workdir", wd])
            res["python_witness"] = child(["--step", "witness", "--file", path])
        print(json.dumps(res, indent=1))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
