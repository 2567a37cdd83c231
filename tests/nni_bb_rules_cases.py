"""The inputs of the tests of the tracked NNI climb under the optional update rules and on a sharded tracker -- shared by the CPU
test (tests/test_nni_bb_rules_witness.py), which asserts on the witness alone that each of them reaches what it is there for, and
the GPU test (tests/test_gpu_nni_bb_rules.py), which runs the same operations on the engine and compares every observable.

A case is a tracker setting and a short list of climbs on ONE tracker; `ops(case)` turns it into operations that `drive` applies to
anything with the engine's method names -- the engine itself, or `WitnessDriver` around a witness.

Alignments: mpboot_amd.synth at 12 x 300 and 24 x 600 DNA (Fitch), 16 x 400 DNA and 12 x 200 protein (weighted): the smallest at
which a climb from a random tree still takes several steps with ties among the samples; start trees and samples as
tests/nni_bb_cases.py makes them.
"""
import functools

import numpy as np

from nni_bb_cases import boot_samples, cutoff_of
from nni_bb_rules_witness import make, make_snk, set_rule, shard_ids
from nni_snk_cases import cost_of


@functools.lru_cache(maxsize=None)
def synth_fx(n, P, alphabet="DNA", seed=1):
    """a fixture dictionary (tests/helpers.py:load_fixture's keys) for a synthetic alignment, one site per pattern"""
    from mpboot_amd import synth
    from oracle import pyoracle as po
    letters, _ = synth.synth_alignment(n, P, alphabet, 0.15, seed=seed)
    codes = synth.letters_to_codes(letters, alphabet)
    dt = 0 if alphabet == "DNA" else 1
    w = np.ones(P, dtype=np.int32)
    inf = np.asarray(po.Oracle(codes, w, datatype=dt).informative()).astype(bool)
    return dict(codes_np=codes, weights_np=w, weights=w.tolist(), datatype=dt, informative=inf.tolist(), S=4 if dt == 0 else 20,
                name=f"synth_{alphabet}_{n}x{P}")


def _c(start, it=1, cut=None, pert=None, speednni=True, steps=50, root=1):
    """one climb: start = seed of the random start tree; it = IQTree::curIt; cut: None | "loose" | "tight" (nni_bb_cases.cutoff_of);
    pert: seed of the re-weighting (a ratchet climb) or None; root: 1 or "n" (the last taxon)"""
    return dict(start=start, it=it, cut=cut, pert=pert, speednni=speednni, steps=steps, root=root)


TWO = [_c(0, 1), _c(1, 2)]                      # two iterations from two random trees
# -distinct_iter_top_boot: two steps of a climb in one iteration, the whole climb in the next (its first trees are the lists' own, the
# later ones beat them: a second representative, then offers that this iteration's representative keeps out), another climb behind
AGAIN = [_c(0, 1, steps=2), _c(0, 2), _c(1, 2)]
AGAIN_CUT = [_c(0, 1, steps=2), _c(0, 2, cut="loose"), _c(1, 2, cut="tight")]
# -storetrees under a matrix that is not symmetric: the first climb's topologies come back from the other root leaf, where a tree's row
# is made at another edge and its length differs -- under a cut-off by then
OTHER_ROOT = [_c(0, 1), _c(0, 2, cut="tight", root="n"), _c(1, 3, cut="tight")]
CUT = [_c(0, 1), _c(1, 2, cut="loose"), _c(2, 3, cut="tight")]
RATCHET = [_c(0, 1, steps=3), _c(1, 2, cut="loose", pert=12345, speednni=False), _c(2, 3)]

# shape: (taxa, patterns); B: samples; rule / arg / store: nni_bb_rules_witness.set_rule; tile: option "nni_tile";
# hclimb1_bb False = -no_hclimb1_bb; shard: None | "interleaved" | "contiguous"; cost (weighted engine): nni_snk_cases.cost_of
FITCH = [
    dict(id="store-12x300-B32", shape=(12, 300), B=32, rule="default", store=True, climbs=CUT, tile=-1),
    dict(id="store-mulhits-24x600-B32-tile2", shape=(24, 600), B=32, rule="mulhits", store=True, climbs=CUT, tile=2),
    dict(id="store-ratchet-12x300-B64", shape=(12, 300), B=64, rule="default", store=True, climbs=RATCHET, tile=-1),
    dict(id="topboot1-12x300-B32", shape=(12, 300), B=32, rule="topboot", arg=1, climbs=TWO, tile=-1),
    dict(id="topboot3-24x600-B64-tile1", shape=(24, 600), B=64, rule="topboot", arg=3, climbs=TWO, tile=1),
    dict(id="topboot3-store-cut-12x300-B32", shape=(12, 300), B=32, rule="topboot", arg=3, store=True, climbs=CUT, tile=-1),
    dict(id="topboot3-ratchet-12x300-B32", shape=(12, 300), B=32, rule="topboot", arg=3, climbs=RATCHET, tile=-1),
    dict(id="topboot1-ratchet-no_hclimb1_bb-12x300-B32", shape=(12, 300), B=32, rule="topboot", arg=1, climbs=RATCHET, tile=-1, hclimb1_bb=False),
    dict(id="distinct1-12x300-B32", shape=(12, 300), B=32, rule="distinct", arg=1, climbs=TWO, tile=-1),
    dict(id="distinct2-24x600-B64-tile2", shape=(24, 600), B=64, rule="distinct", arg=2, climbs=AGAIN, tile=2),
    dict(id="distinct2-store-cut-12x300-B32", shape=(12, 300), B=32, rule="distinct", arg=2, store=True, climbs=AGAIN_CUT, tile=-1),
    dict(id="distinct2-ratchet-12x300-B64", shape=(12, 300), B=64, rule="distinct", arg=2, climbs=RATCHET, tile=1),
    dict(id="distinct1-ratchet-no_hclimb1_bb-12x300-B32", shape=(12, 300), B=32, rule="distinct", arg=1, climbs=RATCHET, tile=-1, hclimb1_bb=False),
]

WEIGHTED = [
    dict(id="snk-store-tstv-16x400-B32", shape=(16, 400), B=32, cost="tstv", rule="default", store=True, climbs=CUT),
    dict(id="snk-store-asym-16x400-B32", shape=(16, 400), B=32, cost="asym", rule="default", store=True, climbs=OTHER_ROOT),
    dict(id="snk-topboot3-asym-16x400-B64", shape=(16, 400), B=64, cost="asym", rule="topboot", arg=3, climbs=TWO),
    dict(id="snk-topboot1-store-ratchet-tstv-16x400-B32", shape=(16, 400), B=32, cost="tstv", rule="topboot", arg=1, store=True, climbs=RATCHET),
    dict(id="snk-distinct2-tstv-16x400-B32", shape=(16, 400), B=32, cost="tstv", rule="distinct", arg=2, climbs=AGAIN),
    dict(id="snk-distinct1-cut-asym-16x400-B32", shape=(16, 400), B=32, cost="asym", rule="distinct", arg=1, climbs=CUT),
    dict(id="snk-distinct2-aa-12x200-B32", shape=(12, 200), alphabet="AA", B=32, cost="metric", rule="distinct", arg=2, climbs=AGAIN),
]

SHARDED = [
    dict(id="shard-default-interleaved-12x300-B130", shape=(12, 300), B=130, rule="default", climbs=CUT, shard="interleaved"),
    dict(id="shard-store-contiguous-12x300-B130", shape=(12, 300), B=130, rule="default", store=True, climbs=TWO, shard="contiguous"),
    dict(id="shard-topboot3-contiguous-24x600-B64", shape=(24, 600), B=64, rule="topboot", arg=3, climbs=TWO, shard="contiguous"),
    dict(id="shard-distinct2-ratchet-interleaved-12x300-B32", shape=(12, 300), B=32, rule="distinct", arg=2, climbs=RATCHET, shard="interleaved"),
    dict(id="shard-snk-topboot1-asym-interleaved-16x400-B32", shape=(16, 400), B=32, cost="asym", rule="topboot", arg=1, climbs=TWO, shard="interleaved"),
    dict(id="shard-snk-mulhits-store-tstv-contiguous-16x400-B130", shape=(16, 400), B=130, cost="tstv", rule="mulhits", store=True, climbs=CUT,
         shard="contiguous"),
]

ALL = FITCH + WEIGHTED + SHARDED


def by_id(case_id):
    return next(c for c in ALL if c["id"] == case_id)


def fixture(case):
    n, P = case["shape"]
    return synth_fx(n, P, case.get("alphabet", "DNA"))


def samples_of(case):
    fx = fixture(case)
    return boot_samples(len(fx["weights"]), case["B"], 7 + case["B"], fx["weights"])


def cost_matrix(case):
    return None if "cost" not in case else cost_of(case["cost"], fixture(case)["S"])


def new_witness(case, shards=None):
    fx = fixture(case)
    cost = cost_matrix(case)
    w = make(fx, 11, samples_of(case)) if cost is None else make_snk(fx, cost, 11, samples_of(case))
    set_rule(w, case["rule"], case.get("arg", 0), case.get("store", False))
    w.ratchet_booking = case.get("hclimb1_bb", True)
    w.shards = shards
    return w


def ops(case):
    """-> [(name, arguments)]: set_weights / ufboot_set_cutoff / ufboot_set_iteration / set_tree / ufboot_optimize_nni.  The cut-off of
    a climb comes from its start tree's length on the original weights alone"""
    from mpboot_amd import engine, trees
    fx = fixture(case)
    n = fx["codes_np"].shape[0]
    ruler = new_witness(case)
    out = []
    for c in case["climbs"]:
        back = trees.random_topology(n, np.random.default_rng(100 + c["start"]))
        w = fx["weights_np"]
        if c["pert"] is not None:
            w, _st = engine.iq_perturb_weights(fx["weights_np"], fx["informative"], 50, 1, c["pert"])
            assert (w != fx["weights_np"]).any() and not ((fx["weights_np"] > 0) & (w <= 0)).any()
        out.append(("set_weights", (np.asarray(w, dtype=np.int32),)))
        out.append(("ufboot_set_cutoff", (cutoff_of(c["cut"], ruler.length([int(x) for x in back])),)))
        out.append(("ufboot_set_iteration", (c["it"],)))
        out.append(("set_tree", (back,)))
        out.append(("ufboot_optimize_nni", (n if c["root"] == "n" else 1, c["speednni"], c["steps"])))
    return out


class WitnessDriver:
    """a witness under the engine's method names"""

    def __init__(self, w):
        self.w = w

    def set_weights(self, wgt):
        self.w.set_weights(wgt)

    def ufboot_set_cutoff(self, x):
        self.w.cutoff = x

    def ufboot_set_iteration(self, it):
        self.w.cur_it = it

    def set_tree(self, back):
        self.w.set_tree(back)

    def ufboot_optimize_nni(self, root, speednni, steps):
        self.w.root = root
        self.w.cur_climb += 1
        return self.w.optimize_nni(speednni, steps)


def drive(target, case, after=None):
    """apply the case's operations; -> the climbs' results.  after(index of the climb): called behind every climb"""
    res = []
    for name, args in ops(case):
        r = getattr(target, name)(*args)
        if name == "ufboot_optimize_nni":
            res.append(tuple(int(x) for x in r))
            if after:
                after(len(res) - 1)
    return res


@functools.lru_cache(maxsize=None)
def climbed(case_id, sharded=False):
    """the witness after the case's climbs, made once and never changed afterwards: -> (witness, results, per climb a snapshot of
    its books).  sharded: the two-shard mode with the case's split"""
    case = by_id(case_id)
    w = new_witness(case, shard_ids(case["B"], case["shard"]) if sharded else None)
    snaps = []
    res = drive(WitnessDriver(w), case, after=lambda _i: snaps.append(snapshot(w)))
    return w, res, snaps


def snapshot(w):
    """every observable of the books, as plain data"""
    return dict(treels_logl=list(w.treels_logl), boot_logl=list(w.boot_logl), boot_counts=list(w.boot_counts), boot_trees=list(w.boot_trees),
                boot_sets=[sorted(s) for s in w.boot_sets], boot_top=[list(t) for t in w.boot_top], boot_top_iter=[list(t) for t in w.boot_top_iter],
                boot_threshold=list(w.boot_threshold), duplicates=w.duplicates, ufb_draws=w.ufb_draws, rng=int(w.rng.state),
                back=list(w.back), log=list(w.log), calls=w.live_calls)


# ---- the sequence test: an SPR tracked climb, a tracked NNI climb, SPR again, on one tracker under -mulhits -topboot 3.  On the
# tests' dna_ambig alignment (14 taxa), the NNI climb from a stepwise-addition tree: from there it reaches trees that beat entries of
# the lists the radius-1 SPR climb from a random tree has left, so every one of the three calls changes the lists
SEQUENCE = dict(id="sequence", B=32, rule="topboot", arg=3,
                calls=[("spr", ("random", 8), 1), ("nni", ("stepwise", 1), 0), ("spr", ("random", 10), 2)])


def sequence_inputs():
    from helpers import load_fixture
    from nni_bb_cases import start_tree
    fx = load_fixture("dna_ambig")
    samples = boot_samples(len(fx["weights"]), SEQUENCE["B"], 5, fx["weights"])
    return fx, samples, [(kind, start_tree(fx, start), radius) for kind, start, radius in SEQUENCE["calls"]]


@functools.lru_cache(maxsize=None)
def sequence_witness():
    """-> (witness, per call its result and a snapshot of the books); made once, never changed"""
    fx, samples, calls = sequence_inputs()
    w = make(fx, 11, samples)
    set_rule(w, SEQUENCE["rule"], SEQUENCE["arg"])
    out = []
    for kind, back, radius in calls:
        w.set_tree(back)
        r = w.optimize(1, radius) if kind == "spr" else WitnessDriver(w).ufboot_optimize_nni(1, True, 50)
        out.append((r, snapshot(w)))
    return w, out
