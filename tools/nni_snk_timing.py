"""Time of the weighted NNI-scoring kernel k_snk_nni_eval next to the Fitch kernel k_nni_eval, DESIGN §5j.

    python tools/nni_snk_timing.py --out profiles/nni_snk_timing.json          # C2 and C5

Per workload one random topology, one full evaluation (every inner branch, both moves) per launch.  Kernel times are HIP events
around the launch inside the engine (option "timing", read-only option "nni_kernel_ns"): 5 launches of warm-up, then the mean of
`--launches` (at least 20) launches.  Reported per launch and per (branch, kept pattern), for
  * k_nni_eval on a Fitch engine over the same alignment and tree,
  * k_snk_nni_eval with packed 16-bit costs and with 32-bit costs (option "sankoff_short"), under a symmetric metric matrix,
and next to the 16-bit figure the packed-u16 VALU ceiling of the same launch: the kernel's packed add / min instructions per wave
at the measured issue rate of v_pk_add_u16 / v_pk_min_u16, 1.76 ns per wave-instruction and SIMD (profiles/r3/valu_rate.txt, the
figure DESIGN uses for k_snk_scan), on 256 CUs x 4 SIMDs.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpboot_amd import engine, synth, trees  # noqa: E402

PK_NS = 1.76            # ns per packed 16-bit add / min wave-instruction and SIMD
SIMDS = 256 * 4


def metric(S, seed=4):
    pts = np.random.default_rng(seed).integers(0, 12, size=(S, 3))
    c = np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2).astype(np.uint32)
    c[c == 0] = 1
    np.fill_diagonal(c, 0)
    return c


def per_launch_ns(e, launches):
    for _ in range(5):
        e.nni_scores(1)
    t0 = e.get_option("nni_kernel_ns")
    for _ in range(launches):
        a, _b, _ln = e.nni_scores(1)
    return (e.get_option("nni_kernel_ns") - t0) / launches, len(a)


def pk_instructions_per_wave(S):
    """both moves: X (S adds), m(X) (S*S adds, S*S mins counting the first as a move), the minimum over Y + m(X) (2 S adds, S mins)"""
    return 2 * (S + 2 * S * S + 3 * S)


def run(workloads, launches, out_path):
    out = {}
    for wl in workloads:
        cfg = synth.WORKLOADS[wl]
        letters, _ = synth.workload(wl)
        codes = synth.letters_to_codes(letters, cfg["alphabet"])
        protein = cfg["alphabet"] == "AA"
        dt = engine.AA if protein else engine.DNA
        S = 20 if protein else 4
        n = codes.shape[0]
        back = trees.random_topology(n, np.random.default_rng(5))
        r = {"n": n, "launches": launches}
        f = engine.FitchEngine(codes, datatype=dt)
        f.set_option("timing", 1)
        f.set_tree(back)
        ns, nb = per_launch_ns(f, launches)
        r["branches"] = nb
        r["k_nni_eval"] = {"us_per_launch": ns / 1e3, "kept_patterns": f.num_informative,
                           "ps_per_branch_pattern": ns * 1e3 / (nb * f.num_informative)}
        f.close()
        w = engine.FitchEngine(codes, datatype=dt, cost=metric(S))
        w.set_option("timing", 1)
        w.set_option("nni_weighted", 1)
        for short, key in ((1, "k_snk_nni_eval_u16"), (0, "k_snk_nni_eval_u32")):
            w.set_option("sankoff_short", short)
            w.set_tree(back)
            ns, nb2 = per_launch_ns(w, launches)
            assert nb2 == nb
            kept = w.num_informative
            d = {"us_per_launch": ns / 1e3, "kept_patterns": kept, "ps_per_branch_pattern": ns * 1e3 / (nb * kept)}
            if short:
                waves = nb * ((w.Wp // 2 + 63) // 64)
                ceil_ns = waves * pk_instructions_per_wave(S) * PK_NS / SIMDS
                d["pk_u16_valu_ceiling_us"] = ceil_ns / 1e3
                d["fraction_of_ceiling"] = ceil_ns / ns if ns else None
            r[key] = d
        w.close()
        out[wl] = r
        print(wl, json.dumps(r), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["C2", "C5"])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a.workloads, max(20, a.launches), a.out)
