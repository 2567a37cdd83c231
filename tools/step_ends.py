#!/usr/bin/env python3
"""The two ends of a from-scratch sweep step at C3 (set_tree + sweep_scan(1, 6), plan_cache 0): what the host spends in front of
the step's first launch and behind its last flag, and how long the GPU stands idle between two steps.

  tools/step_ends.py [--steps 50] [--opt key=value ...] [--no-trace]

  counters  engine.stats() host_front_ms_total (entry of mpf_set_tree .. return of the sweep's first kernel launch) and
            host_behind_ms_total (the minima's flag seen .. return of mpf_sweep_scan), per step, in a process of its own
            (options host_front_ns_total / host_behind_ns_total of the library, booked with timing >= 1)
  gap       from a rocprofv3 --kernel-trace run of its own (the program behind --, no counters): the time from the end of a step's
            k_part_min to the start of the next kernel of the engine, per step; and the kernels that stand between k_part_min and the
            next refresh

MPF_LIB_PATH names another build of the library (a library from before the counters reports them as zero)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def steps(n_steps, opts, quiet):
    import numpy as np
    from mpboot_amd import engine, synth
    letters, _names = synth.workload("C3")
    codes = synth.letters_to_codes(letters, "DNA")
    e = engine.FitchEngine(codes, datatype=engine.DNA)
    e.set_option("timing", 1)
    for kv in opts:
        k, v = kv.split("=")
        e.set_option(k, int(v))
    e.seed_ties(engine.TIE_RANDOM, 1)
    e.make_parsimony_tree(12345, 0)
    back = e.get_tree()
    e.set_option("plan_cache", 0)
    for _ in range(10):
        e.set_tree(back)
        e.sweep_scan(1, 6)
    front, behind, wall = [], [], []
    for _ in range(n_steps):
        e.reset_stats()
        t0 = time.perf_counter()
        e.set_tree(back)
        k, best = e.sweep_scan(1, 6)
        wall.append((time.perf_counter() - t0) * 1e6)
        st = e.stats()
        front.append(st.get("host_front_ms_total", 0.0) * 1e3)
        behind.append(st.get("host_behind_ms_total", 0.0) * 1e3)
    if not quiet:
        for i in range(n_steps):
            print(f"step {i:3d}: host_front {front[i]:7.1f} us  host_behind {behind[i]:7.1f} us  step {wall[i]:7.1f} us")
    try:
        active = e.get_option("sweep_ends_active")
    except Exception:
        active = None                               # (a library from before the option)
    res = {"steps": n_steps, "tests": int(k), "best": int(best), "sweep_ends_active": active,
           "host_front_us": {"median": statistics.median(front), "min": min(front), "max": max(front)},
           "host_behind_us": {"median": statistics.median(behind), "min": min(behind), "max": max(behind)},
           "step_us": {"median": statistics.median(wall), "min": min(wall), "max": max(wall)}}
    print(json.dumps(res))
    return res


def short(name):
    return name.replace("void mpf::", "").replace("mpf::", "").split("(")[0].split("<")[0]


def traced(n_steps, opts, limit):
    """the idle time between two steps, from a kernel trace of a run of its own"""
    with tempfile.TemporaryDirectory() as wd:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", wd, "--",
               sys.executable, os.path.abspath(__file__), "--child", "--quiet", "--steps", str(n_steps)]
        for kv in opts:
            cmd += ["--opt", kv]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("the traced run ended with status %d: stopping here" % r.returncode)
        files = glob.glob(os.path.join(wd, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return {"note": "rocprofv3 wrote no kernel_trace.csv"}
        rows = []
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), short(row["Kernel_Name"])))
    rows.sort()
    last = [i for i, x in enumerate(rows) if x[2] == "k_part_min"][-n_steps:]      # the timed steps are the last ones
    gaps, between, dur = [], {}, {}
    for i in last:
        if i + 1 >= len(rows):
            continue
        gaps.append((rows[i + 1][0] - rows[i][1]) / 1e3)
        j = i + 1
        names = []
        while j < len(rows) and not rows[j][2].startswith("k_newview"):
            names.append(rows[j][2])
            j += 1
        key = ",".join(names) if names else "-"
        between[key] = between.get(key, 0) + 1
    for s, t, name in rows[last[0] if last else 0:]:
        dur.setdefault(name, []).append((t - s) / 1e3)
    res = {"traced_steps": len(gaps),
           "gap_us": {"median": statistics.median(gaps), "min": min(gaps), "max": max(gaps)} if gaps else None,
           "kernels_between_part_min_and_refresh": between,
           "kernel_us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2), "n": len(v)} for k, v in sorted(dur.items())}}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--opt", action="append", default=[], help="engine option key=value")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help="(the steps alone, in this process)")
    ap.add_argument("--quiet", action="store_true", help="(with --child: no line per step)")
    ap.add_argument("--trace-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        steps(a.steps, a.opt, a.quiet)
    else:
        # (each part in a process of its own: this one never opens the GPU)
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps)]
        for kv in a.opt:
            cmd += ["--opt", kv]
        r = subprocess.run(cmd)
        if r.returncode != 0:
            raise SystemExit("the counters' run ended with status %d: stopping here" % r.returncode)
        if not a.no_trace:
            traced(a.steps, a.opt, a.trace_timeout)
