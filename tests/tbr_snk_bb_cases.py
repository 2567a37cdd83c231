"""The inputs of the weighted tracked TBR sweep's and climb's tests -- shared by the CPU test, which asserts that each of them really
exercises the tracker's update rule, and the GPU test, which compares the engine with the witness on them
(tests/tbr_snk_bb_witness.py).

Random patterns with nothing tree-like in them (tests/tbr_witness.py:alignment, weights 1 .. 5, every pattern kept), a random start
tree and a symmetric cost matrix (tests/nni_snk_cases.py: tstv for DNA, a random metric for the protein and the 32-state case).  The
seeds were picked by a search on the CPU (the first seed from 0 at which the case shows what tests/test_tbr_snk_bb_witness.py asks of
it, on the witness alone) and are pinned here.

FormB: the same bookkeeping over the witness's VECTORISED form (b) -- directed views, chains, root sets, one min-plus join per entry
-- for the one GPU shape that form (a) would take too long for; the CPU test ties it to form (a) row by row and book by book."""
import numpy as np

import tbr_witness as tw
from mpboot_amd import trees
from nni_snk_cases import cost_of
from tbr_bb_cases import boot_samples, cutoff_of
from tbr_snk_bb_witness import RowScorer, TbrSnkBbWitness

DT = {"dna": 0, "aa": 1, "m32": 3}
STATES = {"dna": 4, "aa": 20, "m32": 32}
KIND = {"dna": "tstv", "aa": "metric", "m32": "metric"}
# alphabet -> (taxa, patterns, samples, radius, moves of a climb at most)
SIZES = {"dna": (14, 150, 16, 2, 3), "aa": (10, 61, 8, 3, 2), "m32": (8, 33, 16, 3, 2)}
RULES = ("default", "cut", "mulhits", "btrees")
SEEDS = {
    ("dna", "default", "sweep"): 0, ("dna", "cut", "sweep"): 0, ("dna", "mulhits", "sweep"): 0, ("dna", "btrees", "sweep"): 0,
    ("dna", "default", "climb"): 0, ("dna", "cut", "climb"): 0, ("dna", "mulhits", "climb"): 0, ("dna", "btrees", "climb"): 0,
    ("aa", "default", "sweep"): 0, ("aa", "cut", "sweep"): 0, ("aa", "mulhits", "sweep"): 1, ("aa", "btrees", "sweep"): 0,
    ("aa", "default", "climb"): 0, ("aa", "cut", "climb"): 0, ("aa", "mulhits", "climb"): 0, ("aa", "btrees", "climb"): 0,
    ("m32", "default", "sweep"): 0, ("m32", "cut", "sweep"): 0, ("m32", "mulhits", "sweep"): 0, ("m32", "btrees", "sweep"): 0,
    ("m32", "default", "climb"): 0, ("m32", "cut", "climb"): 0, ("m32", "mulhits", "climb"): 0, ("m32", "btrees", "climb"): 0,
}
CASES = [dict(id=f"{a}-{r}-{k}", alphabet=a, rule=r, kind=k, seed=SEEDS[(a, r, k)])
         for a in ("dna", "aa", "m32") for r in RULES for k in ("sweep", "climb")]


def matrix_of(alphabet, seed=0):
    return cost_of(KIND[alphabet], STATES[alphabet], seed=4 + seed)


def make(codes, weights, alphabet, cost, tie_seed, samples=None, cls=TbrSnkBbWitness):
    return cls(codes, weights, DT[alphabet], cost, tie_seed, samples)


def setup(case, seed=None, cls=TbrSnkBbWitness, sizes=None):
    """-> (codes, weights, cost matrix, start back[], samples, radius, max_moves, witness ready to run, cut-off)"""
    a, seed = case["alphabet"], case["seed"] if seed is None else seed
    n, P, B, radius, max_moves = sizes or SIZES[a]
    codes, weights = tw.alignment(n, P, a, 500 + seed)
    cost = matrix_of(a, seed)
    back = trees.random_topology(n, np.random.default_rng(700 + seed))
    samples = boot_samples(weights, B, 900 + seed)
    w = make(codes, weights, a, cost, 11 + seed, samples, cls)
    w.set_tree(back)
    w.mulhits = case["rule"] == "mulhits"
    w.cutoff_from_btrees = case["rule"] == "btrees"
    w.cutoff = cutoff_of(case["rule"], w.length(w.back))
    return codes, weights, cost, back, samples, radius, max_moves, w, w.cutoff


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


# ---- form (b) with its rows: what the engine's kernel computes, in numpy
def visit_rows(sc, back, p, maxtrav, views):
    """(F records, G records, rows[1 + |F|][1 + |G|][P]) of one visit: min_x( RF_i[x] + m(RG_j)[x] ) per kept pattern, scattered to
    all patterns"""
    q = int(back[p])
    F, G = tw.lists(back, sc.n, p, maxtrav)
    rf = np.stack([views[q][0]] + sc.root_sets(back, views, q, maxtrav))
    mrg = np.stack([views[p][1]] + [sc.m(r) for r in sc.root_sets(back, views, p, maxtrav)])
    rows = np.zeros((len(rf), len(mrg), sc.P), dtype=np.int64)
    for i in range(len(rf)):
        rows[i][:, sc.cols] = np.min(rf[i][None, :, :] + mrg, axis=1)
    return [r for r, _ in F], [r for r, _ in G], rows


class FormB(TbrSnkBbWitness):
    """TbrSnkBbWitness with every entry's length and row from form (b); the tree of an entry is built only to be booked"""

    def pattern_lengths(self, back):
        return self.entry_row if self.entry_row is not None else TbrSnkBbWitness.pattern_lengths(self, back)

    entry_row = None

    def sweep_best(self, back, maxtrav, spr_only=False):
        assert not spr_only
        back = np.array(back, dtype=np.int32)
        views, out, pairs = self.scorer.views(back), [], 0
        wts = self.scorer.w.w
        for v, p in enumerate(tw.node_order(back, self.n)):
            F, G, rows = visit_rows(self.scorer, back, p, maxtrav, views)
            fr, gr = [tw.NONE] + F, [tw.NONE] + G
            cost = rows[:, :, self.scorer.cols] @ wts
            for i, f in enumerate(fr):
                for j, g in enumerate(gr):
                    self.back = [int(x) for x in trees.apply_tbr(back, p, f, g)]
                    self.entry_row = rows[i, j]
                    before = len(self.treels_logl) if self.bb else 0
                    self.book_entry(int(cost[i, j]), "cur" if i == 0 and j == 0 else "cand", (v, i, j))
                    if self.bb and len(self.treels_logl) > before:
                        self.rows.append(((v, i, j), int(cost[i, j]), self.pattern_pars.copy()))
            self.entry_row = None
            pairs += cost.size
            best = tw.first_min(cost)
            out.append((tw.NO_BEST, tw.NONE, tw.NONE) if best is None else (int(best[0]), fr[best[1]], gr[best[2]]))
        self.back = [int(x) for x in back]
        return out, pairs


# ---- the one shape above a single tile per row with 20 states (tests/test_gpu_tbr_snk_bb.py): 36 taxa x 260 patterns (130 elements
# in the 16-bit store), radius 2, 16 samples, one sweep, on FormB
BIG = dict(alphabet="aa", rule="default", kind="sweep", seed=0)
BIG_SIZES = (36, 260, 16, 2, 0)


# ---- the hand-over: a weighted tracked SPR climb, a TBR tracked sweep, a weighted tracked NNI climb on one tracker
HANDOVER = dict(fx="dna_clean", cost="tstv", B=8, sseed=4, tie=13, starts=(8, 9, 10), spr_radius=2, tbr_radius=2)
