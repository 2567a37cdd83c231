"""Time of the Robinson-Foulds distances on the device next to the host-only program, DESIGN 5n.

    python tools/rf_timing.py --out profiles/rf/timing.json

Two shapes, all pairs: the 5m shape (1000 trees x 1000 taxa, each 0 .. 16 local SPR moves from one tree) and a wide one in which
the product dominates (4096 trees x 500 taxa, 0 .. 64 moves).  The tree sets are made as tools/splits_timing.py makes them.  Steps,
each a child process of its own, every one that opens the GPU under `timeout`; a step that fails ends the run:

  gpu    mpf_rf_distances, the whole call (wall clock: staging, split pass, rows, product, the copy of the result), after a warm-up,
         `--reps` times: median, minimum and maximum.  In a second run of the same call under the option "timing" the HIP-event times
         of the kernels inside it: split_keys_ns + split_count_ns (the split pass), rf_rows_ns (k_rf_rows + k_rf_patch),
         rf_shared_ns; and rf_columns, rf_chunks.  For k_rf_shared the and + bcnt pairs per second it achieved -- tiles x 64 x 64 x padded words -- next to the
         VALU issue bound: 256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz / 2 instructions per pair.
  host   mpboot_amd/host/rf_host_main.cpp built with -O2 and without a sanitizer, fed the same trees: ms_rf, the host's own exact
         distances on one core, median of 3
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from splits_timing import make_trees  # noqa: E402

SHAPES = (("bb_1000x1000", 1000, 1000, 16), ("wide_4096x500", 500, 4096, 64))
VALU_PAIR_BOUND = 256 * 4 * 32 * 2.4e9 / 2
TILE, K_STEP = 64, 32


def load(path):
    with open(path, "rb") as f:
        n, _mode, T, _T2 = np.fromfile(f, dtype=np.int32, count=4)
        return int(n), np.fromfile(f, dtype=np.int32).reshape(int(T), -1)


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def step_gpu(path, reps):
    from mpboot_amd import engine
    n, backs = load(path)
    codes = (1 << np.random.default_rng(1).integers(0, 4, size=(n, 64))).astype(np.uint8)
    e = engine.FitchEngine(codes)
    for _ in range(2):
        rf = e.rf_distances(backs)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rf = e.rf_distances(backs)
        wall.append((time.perf_counter() - t0) * 1e3)
    out = {"whole_call": spread(wall), "rf_columns": e.get_option("rf_columns"), "rf_chunks": e.get_option("rf_chunks"),
           "rf_launches": e.get_option("rf_launches"), "overflow": e.get_option("split_overflow"),
           "mean_rf": float(rf.sum()) / max(1, rf.size - len(rf)), "max_rf": int(rf.max())}
    e.set_option("timing", 1)
    e.rf_distances(backs)
    keys, rows, shared = [], [], []
    for _ in range(reps):
        k0 = e.get_option("split_keys_ns") + e.get_option("split_count_ns")
        e.rf_distances(backs)
        keys.append((e.get_option("split_keys_ns") + e.get_option("split_count_ns") - k0) / 1e6)
        rows.append(e.get_option("rf_rows_ns") / 1e6)
        shared.append(e.get_option("rf_shared_ns") / 1e6)
    T = len(backs)
    nt = -(-T // TILE)
    words = -(-(-(-out["rf_columns"] // 32)) // K_STEP) * K_STEP if out["rf_chunks"] == 1 else None
    out["kernels"] = {"split_pass": spread(keys), "k_rf_rows": spread(rows), "k_rf_shared": spread(shared)}
    if words:
        pairs = nt * (nt + 1) // 2 * TILE * TILE * words
        rate = pairs / (statistics.median(shared) * 1e-3)
        out["k_rf_shared_rate"] = {"tiles": nt * (nt + 1) // 2, "padded_words_per_row": words, "and_bcnt_pairs": pairs,
                                   "pairs_per_s": rate, "valu_issue_bound_pairs_per_s": VALU_PAIR_BOUND,
                                   "fraction_of_bound": rate / VALU_PAIR_BOUND}
    print(json.dumps(out))


def step_host(path, workdir):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(workdir, "rf_host")
    if not os.path.exists(exe):
        subprocess.check_call([cxx, "-std=c++17", "-O2", os.path.join(ROOT, "mpboot_amd", "host", "rf_host_main.cpp"), "-o", exe])
    ms, tail = [], {}
    for _ in range(3):
        r = subprocess.run([exe, "rf", path, "quiet"], capture_output=True, text=True, check=True)
        tail = {ln.split()[0]: ln.split()[1] for ln in r.stdout.splitlines()}
        ms.append(float(tail["ms_rf"]))
    print(json.dumps({"ms_rf": spread(ms), "entries": int(tail["entries"]), "sum": int(tail["sum"]), "note": "one core, -O2"}))


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
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=[s[0] for s in SHAPES], help="one shape only")
    ap.add_argument("--step", default=None, choices=("gpu", "host"))
    ap.add_argument("--file", default=None)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    if a.step == "gpu":
        step_gpu(a.file, a.reps)
    elif a.step == "host":
        step_host(a.file, a.workdir)
    else:
        res = {"reps": a.reps, "shapes": {}}
        with tempfile.TemporaryDirectory() as wd:
            for name, taxa, T, moves in SHAPES:
                if a.shape and a.shape != name:
                    continue
                path = os.path.join(wd, name + ".bin")
                backs = make_trees(taxa, T, moves, 1)
                with open(path, "wb") as f:
                    np.array([taxa, 0, T, 0], dtype=np.int32).tofile(f)
                    backs.tofile(f)
                one = {"taxa": taxa, "trees": T, "max_moves_per_tree": moves, "mode": "all pairs"}
                one["gpu"] = child(["--step", "gpu", "--file", path, "--reps", str(a.reps)], limit=240)
                one["host_program"] = child(["--step", "host", "--file", path, "--workdir", wd])
                tot = one["host_program"]["sum"]
                one["same_sum_of_distances"] = abs(one["gpu"]["mean_rf"] * (T * T - T) - tot) < 0.5
                res["shapes"][name] = one
                print(json.dumps({name: one}), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
