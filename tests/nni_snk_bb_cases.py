"""The inputs of the tracked weighted NNI climb's tests -- shared by the CPU test, which asserts that each of them really exercises
the tracker's update rule (and that the set holds a kept-worse step and a candidate whose row depends on its edge), and the GPU
test, which compares the engine with the witness on them (tests/nni_snk_bb_witness.py)."""
import functools

import numpy as np

from helpers import load_fixture
from nni_bb_cases import boot_samples, cutoff_of
from nni_snk_bb_witness import make
from nni_snk_cases import cost_of

# cost: "tstv" | "metric" | "asym" (tests/nni_snk_cases.py); start: seed of mpboot_amd.trees.random_topology; root: 1 or "n" (the
# last taxon); cut: None | "loose" | "tight" (nni_bb_cases.cutoff_of, from the start tree's root-leaf length); steps: max_steps
CASES = [
    dict(id="dna_clean-tstv", fx="dna_clean", cost="tstv", start=1, root=1, speednni=True, B=8, sseed=1, tie=3),
    dict(id="dna_ambig-asym-root-n-full", fx="dna_ambig", cost="asym", start=1, root="n", speednni=False, B=8, sseed=2, tie=5, steps=12),
    dict(id="dna_dups-metric-weights", fx="dna_dups", cost="metric", start=2, root=1, speednni=True, B=8, sseed=3, tie=7),
    dict(id="aa-metric", fx="aa", cost="metric", start=0, root=1, speednni=True, B=8, sseed=4, tie=9),
    dict(id="dna_48-asym-mulhits", fx="dna_48", cost="asym", start=0, root=1, speednni=True, B=8, sseed=5, tie=11, rule="mulhits", steps=12),
    dict(id="dna_48-tstv-root-n-full-loose-cut", fx="dna_48", cost="tstv", start=1, root="n", speednni=False, B=8, sseed=6, tie=13, cut="loose", steps=6),
    dict(id="aa_40-asym-root-n-tight-cut", fx="aa_40", cost="asym", start=0, root="n", speednni=True, B=8, sseed=7, tie=15, cut="tight", steps=12),
    dict(id="aa_40-metric-btrees", fx="aa_40", cost="metric", start=3, root=1, speednni=True, B=8, sseed=8, tie=17, btrees=True),
    dict(id="morph32-metric", fx="morph32", cost="metric", start=2, root=1, speednni=True, B=8, sseed=9, tie=19),
    dict(id="dna_clean-asym-mulhits-tight-cut", fx="dna_clean", cost="asym", start=3, root=1, speednni=True, B=8, sseed=10, tie=21, rule="mulhits",
         cut="tight", steps=12),
]


def start_tree(fx, seed):
    from mpboot_amd import trees
    return trees.random_topology(fx["codes_np"].shape[0], np.random.default_rng(seed))


def setup(case):
    """-> (fixture, cost matrix, n, root taxon, start back[], samples, witness ready to climb, cut-off)"""
    fx = load_fixture(case["fx"])
    n = fx["codes_np"].shape[0]
    cost = cost_of(case["cost"], fx["S"])
    root = n if case["root"] == "n" else 1
    back = start_tree(fx, case["start"])
    samples = boot_samples(len(fx["weights"]), case["B"], case["sseed"], fx["weights"])
    w = make(fx, cost, case["tie"], samples, root)
    w.set_tree(back)
    w.mulhits = case.get("rule") == "mulhits"
    w.cutoff_from_btrees = case.get("btrees", False)
    w.cutoff = cutoff_of(case.get("cut"), w.length(w.back))
    return fx, cost, n, root, back, samples, w, w.cutoff


@functools.lru_cache(maxsize=None)
def climbed(case_id, max_steps=None):
    """the witness after its climb, made once per (case, step cap): -> (setup tuple, result); nobody changes it afterwards"""
    case = next(c for c in CASES if c["id"] == case_id)
    s = setup(case)
    want = s[6].optimize_nni(speednni=case["speednni"], max_steps=case.get("steps", 50) if max_steps is None else max_steps)
    return s, want
