"""The inputs of the tracked NNI climb's tests -- shared by the CPU test, which asserts that each of them really exercises the
tracker's update rule, and the GPU test, which compares the engine with the witness on them (tests/nni_bb_witness.py)."""
import numpy as np

from helpers import load_fixture
from nni_bb_witness import make
from oracle import pyoracle as po

# start: ("random", seed) = mpboot_amd.trees.random_topology, ("stepwise", seed) = the oracle's stepwise addition
# root: 1 or "n" (the last taxon); cut: None | "loose" (trees no longer than the start tree) | "tight" (see cutoff_of)
# The four rollback starts are those of tests/test_gpu_nni.py::test_rollback_path.
CASES = [
    dict(id="dna_clean-random", fx="dna_clean", start=("random", 0), root=1, speednni=True, B=8, sseed=1, tie=3),
    dict(id="dna_ambig-stepwise-keepall", fx="dna_ambig", start=("stepwise", 1), root="n", speednni=False, B=8, sseed=2, tie=5, keep_all=True),
    dict(id="dna_dups-rollback", fx="dna_dups", start=("random", 1), root=1, speednni=True, B=8, sseed=3, tie=7),
    dict(id="aa-random", fx="aa", start=("random", 0), root=1, speednni=True, B=8, sseed=4, tie=9),
    dict(id="dna_48-mulhits", fx="dna_48", start=("random", 0), root=1, speednni=False, B=8, sseed=5, tie=11, rule="mulhits"),
    dict(id="bin-rollback-loose-cut", fx="bin", start=("random", 0), root=1, speednni=True, B=8, sseed=6, tie=13, cut="loose"),
    dict(id="bin-rollback-full-root-n", fx="bin", start=("random", 2), root="n", speednni=False, B=8, sseed=7, tie=15),
    dict(id="morph-rollback-btrees", fx="morph", start=("random", 0), root=1, speednni=True, B=8, sseed=8, tie=17, btrees=True),
    dict(id="morph32-random", fx="morph32", start=("random", 2), root=1, speednni=True, B=8, sseed=9, tie=19),
    dict(id="morph32_40-stepwise", fx="morph32_40", start=("stepwise", 1), root=1, speednni=True, B=8, sseed=2, tie=5),
    dict(id="morph32_40-tight-cut", fx="morph32_40", start=("random", 2), root=1, speednni=True, B=8, sseed=10, tie=21, cut="tight"),
    dict(id="aa_40-keepall-full", fx="aa_40", start=("random", 0), root="n", speednni=False, B=8, sseed=11, tie=23, keep_all=True),
    dict(id="dna_clean-mulhits-tight-cut", fx="dna_clean", start=("random", 3), root=1, speednni=True, B=8, sseed=12, tie=25, rule="mulhits",
         cut="tight"),
]


def boot_samples(P, B, seed, weights):
    rng = np.random.default_rng(seed)
    w = np.asarray(weights, dtype=np.float64)
    return rng.multinomial(int(w.sum()), w / w.sum(), size=B).astype(np.uint16)


def start_tree(fx, start, keep_all=False):
    from mpboot_amd import trees
    kind, seed = start
    n = fx["codes_np"].shape[0]
    if kind == "random":
        return trees.random_topology(n, np.random.default_rng(seed))
    o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], keep_all=keep_all)
    o.stepwise(seed)
    return o.get_tree()


def cutoff_of(kind, start_len):
    """logl_cutoff from the start tree's length alone: "loose" books the trees no longer than the start tree, "tight" those at
    least 3 % shorter -- early steps have candidates on both sides, later ones pass whole"""
    if kind is None:
        return 0.0
    return -float(start_len) if kind == "loose" else -float(int(start_len * 0.97))


def setup(case):
    """-> (fixture, n, root taxon, start back[], samples, witness ready to climb, cut-off)"""
    fx = load_fixture(case["fx"])
    n = fx["codes_np"].shape[0]
    keep_all = case.get("keep_all", False)
    root = n if case["root"] == "n" else 1
    back = start_tree(fx, case["start"], keep_all)
    samples = boot_samples(len(fx["weights"]), case["B"], case["sseed"], fx["weights"])
    w = make(fx, case["tie"], samples, root, keep_all)
    w.set_tree(back)
    w.mulhits = case.get("rule") == "mulhits"
    w.cutoff_from_btrees = case.get("btrees", False)
    w.cutoff = cutoff_of(case.get("cut"), w.length(w.back))
    return fx, n, root, back, samples, w, w.cutoff
