"""The inputs of the tracked TBR sweep's and climb's tests -- shared by the CPU test, which asserts that each of them really
exercises the tracker's update rule, and the GPU test, which compares the engine with the witness on them (tests/tbr_bb_witness.py).

Random patterns with nothing tree-like in them (tests/tbr_witness.py:alignment, weights 1 .. 5, every pattern kept) and a random
start tree: a sweep has candidates on both sides of the start tree's length, and a climb moves at once.  The seeds were picked by a
search on the CPU (the first seed from 0 at which the case shows what tests/test_tbr_bb_witness.py asks of it) and are pinned here."""
import numpy as np

import tbr_witness as tw
from mpboot_amd import trees
from tbr_bb_witness import TbrBbWitness

DT = {"dna": 0, "aa": 1, "m32": 3}
# alphabet -> (taxa, patterns, samples, radius, moves of a climb at most)
SIZES = {"dna": (14, 200, 16, 2, 3), "aa": (12, 90, 8, 3, 2), "m32": (10, 40, 32, 3, 2)}
RULES = ("default", "cut", "mulhits", "btrees")
SEEDS = {
    ("dna", "default", "sweep"): 0, ("dna", "cut", "sweep"): 0, ("dna", "mulhits", "sweep"): 0, ("dna", "btrees", "sweep"): 0,
    ("dna", "default", "climb"): 0, ("dna", "cut", "climb"): 0, ("dna", "mulhits", "climb"): 0, ("dna", "btrees", "climb"): 0,
    ("aa", "default", "sweep"): 0, ("aa", "cut", "sweep"): 0, ("aa", "mulhits", "sweep"): 0, ("aa", "btrees", "sweep"): 0,
    ("aa", "default", "climb"): 0, ("aa", "cut", "climb"): 0, ("aa", "mulhits", "climb"): 0, ("aa", "btrees", "climb"): 0,
    ("m32", "default", "sweep"): 0, ("m32", "cut", "sweep"): 0, ("m32", "mulhits", "sweep"): 0, ("m32", "btrees", "sweep"): 0,
    ("m32", "default", "climb"): 0, ("m32", "cut", "climb"): 0, ("m32", "mulhits", "climb"): 0, ("m32", "btrees", "climb"): 0,
}
CASES = [dict(id=f"{a}-{r}-{k}", alphabet=a, rule=r, kind=k, seed=SEEDS[(a, r, k)])
         for a in ("dna", "aa", "m32") for r in RULES for k in ("sweep", "climb")]


def boot_samples(weights, B, seed):
    rng = np.random.default_rng(seed)
    w = np.asarray(weights, dtype=np.float64)
    return rng.multinomial(int(w.sum()), w / w.sum(), size=B).astype(np.uint16)


def cutoff_of(rule, start_len):
    """logl_cutoff from the start tree's length alone: under "cut" the trees no longer than the start tree are booked, so a sweep
    has candidates on both sides; a climb's later sweeps pass more and more of theirs"""
    return -float(start_len) if rule == "cut" else 0.0


def make(codes, weights, alphabet, tie_seed, samples=None):
    return TbrBbWitness(codes, weights, DT[alphabet], np.ones(codes.shape[1], dtype=bool), tie_seed, samples)


def setup(case, seed=None):
    """-> (codes, weights, start back[], samples, radius, max_moves, witness ready to run, cut-off)"""
    a, seed = case["alphabet"], case["seed"] if seed is None else seed
    n, P, B, radius, max_moves = SIZES[a]
    codes, weights = tw.alignment(n, P, a, 500 + seed)
    back = trees.random_topology(n, np.random.default_rng(700 + seed))
    samples = boot_samples(weights, B, 900 + seed)
    w = make(codes, weights, a, 11 + seed, samples)
    w.set_tree(back)
    w.mulhits = case["rule"] == "mulhits"
    w.cutoff_from_btrees = case["rule"] == "btrees"
    w.cutoff = cutoff_of(case["rule"], w.length(w.back))
    return codes, weights, back, samples, radius, max_moves, w, w.cutoff


def run(case, w, radius, max_moves):
    """the witness's side of a case -> what the engine's call must return"""
    if case["kind"] == "sweep":
        return w.tbr_sweep(radius)
    return w.optimize_tbr(radius, max_moves)


def shows_the_rule(case, w, result):
    """what every case must show for its comparison to mean something"""
    ok = w.ufb_draws > 0 or w.mulhits
    ok = ok and w.final_trees_booked_as_interior() > 0
    if case["rule"] == "cut":
        acc, rej = w.candidate_calls()
        ok = ok and acc > 0 and rej > 0
    if case["kind"] == "climb":
        ok = ok and result[1] >= 2
    return ok


# ---- the hand-over: an SPR tracked climb, then a TBR tracked climb, then an NNI tracked climb on one tracker
HANDOVER = dict(fx="dna_ambig", B=8, sseed=4, tie=13, starts=(8, 9, 10), spr_radius=2, tbr_radius=2, tbr_moves=2)


def handover_witness():
    """-> (fixture, samples, start trees, one witness that knows all three climbs)"""
    from helpers import load_fixture
    from nni_bb_cases import boot_samples as fixture_samples, start_tree
    from nni_bb_witness import NniBbWitness

    class AllThree(NniBbWitness, TbrBbWitness):
        pass

    h = HANDOVER
    fx = load_fixture(h["fx"])
    samples = fixture_samples(len(fx["weights"]), h["B"], h["sseed"], fx["weights"])
    w = AllThree(fx["codes_np"], fx["weights_np"], fx["datatype"], np.asarray(fx["informative"], dtype=bool), h["tie"], samples, 1)
    return fx, samples, [start_tree(fx, ("random", s)) for s in h["starts"]], w


def handover_steps(w, starts):
    """the three climbs on the witness -> their results, and treels_logl's size behind each"""
    h, out, sizes = HANDOVER, [], []
    w.set_tree(starts[0])
    out.append(w.optimize(1, h["spr_radius"]))
    sizes.append(len(w.treels_logl))
    w.set_tree(starts[1])
    out.append(w.optimize_tbr(h["tbr_radius"], h["tbr_moves"]))
    sizes.append(len(w.treels_logl))
    w.set_tree(starts[2])
    out.append(w.optimize_nni(True))
    sizes.append(len(w.treels_logl))
    return out, sizes
