"""Witness of mpboot's NNI hill climb under a cost matrix and -bb (-cost m -nni_pars -bb, save_all_trees == 2) -- TEST
INFRASTRUCTURE ONLY.

Under -cost the tree is a ParsTree.  A scoring step of IQTree::optimizeNNI (reference iqtree.cpp:2178-2295) hands 1 + 2 * branches
trees to saveCurrentTree: the current tree with curScore (:2181-2183), then move 0 and move 1 of every evaluated branch in
evaluation order (phylotree.cpp:3907-3939).  pllComputePatternParsimony is not called on this path (iqtree.cpp:3363), so
_pattern_pars is what ParsTree::computeParsimonyBranch last wrote (parstree.cpp:460-461, :482-529):

  * for a candidate the per-pattern minima of the branch-rooted scoring, node2's side the parent (`edge_row`);
  * for the current tree the row ParsTree::computeParsimony() wrote at the root-leaf edge (parstree.cpp:101-116, `root_row`).

There is no rollback under -cost (iqtree.cpp:2258): a kept-worse step is followed by an ordinary scoring step that books the current
tree under the longer curScore.

Nothing is copied: the bookkeeping is oracle/search_slow.py:SlowSearch.save_current_tree (as tests/nni_bb_witness.py uses it), the
scoring is tests/nni_snk_witness.py:SnkScorer, and the climb IS SnkNniWitness.optimize -- it asks `score_fn` for the current tree's
length once in front of every step and `score_branch` for every branch it evaluates, in order, so the `book` calls sit in overrides
of those two: the current tree at the first branch of a step, each candidate while its swap is done.  save_current_tree calls
pattern_lengths(back) AFTER the cut-off test; the witness sets the edge before each `book`, which also puts the row into
pattern_pars beforehand, as NniBbWitness.book does (the ratchet length is taken from it).
"""
import numpy as np

from nni_snk_witness import SnkNniWitness, SnkScorer, closed
from oracle.search_slow import SlowSearch


class RowScorer(SnkScorer):
    """SnkScorer with the per-pattern rows behind its two lengths, and 32-state data (one bit per symbol, code 32 = every state:
    bitVector32, globalVariables.h:98-102)"""

    def __init__(self, codes, weights, cost, datatype=0):
        if datatype != 3:
            SnkScorer.__init__(self, codes, weights, cost, protein=datatype == 1)
            return
        SnkScorer.__init__(self, np.zeros_like(codes), weights, np.zeros((4, 4)), protein=False)      # (the caches, the recursion limit)
        self.S = 32
        self.cost = closed(cost).astype(np.int32)
        assert self.cost.shape == (32, 32)
        c = np.asarray(codes, dtype=np.int64)
        sets = np.where(c < 32, np.left_shift(1, np.minimum(c, 31)), (1 << 32) - 1)
        big = int(self.cost.max()) + 1
        self.tips = [np.where((sets[t][None, :] >> np.arange(32)[:, None]) & 1, 0, big).astype(np.int32) for t in range(self.n)]

    def edge_row(self, back, node1, node2):
        """the per-pattern terms of SnkScorer.edge_length"""
        r1 = next(3 * node1 + s for s in range(3 if node1 > self.n else 1) if int(back[3 * node1 + s]) // 3 == node2)
        return np.min(self.view(back, int(back[r1]))[0] + self.view(back, r1)[1], axis=0).astype(np.int64)

    def root_row(self, back, root_taxon=1):
        """... of SnkScorer.length"""
        return np.min(self.view(back, int(back[3 * root_taxon]))[0] + self.view(back, 3 * root_taxon)[1], axis=0).astype(np.int64)


class SnkNniBbWitness(SlowSearch, SnkNniWitness):
    def __init__(self, codes, weights, datatype, cost, tie_seed, samples=None, root_taxon=1):
        SlowSearch.__init__(self, codes, weights, datatype, np.ones(codes.shape[1], dtype=bool), tie_seed, samples)
        self.scorer = RowScorer(codes, weights, cost, datatype)
        self.root = root_taxon
        self.score_fn = self._current_length
        self.log = []
        self.rollbacks = 0
        self.kept_worse = 0
        self.most_applied = 0
        self.edge = None                              # the edge _pattern_pars was written at: None = root leaf, else (node1, node2)
        self.step = 0
        self.cur = None                               # (length) of the current tree, to be booked at the step's first branch
        self.calls = []                               # every saveCurrentTree call: (kind, step, booked index or None)
        self.kind_of = {}                             # tree index -> "cur" | "cand"
        self.took = []                                # per call: how many samples' boot_trees entry it changed
        self.rows = []                                # per call: (kind, edge, length it came with, its row, the booked tree's back[])

    # -- scoring: SlowSearch's two entry points on the weighted scorer
    def set_weights(self, w):
        SlowSearch.set_weights(self, w)
        self.scorer.w = self.w.copy()

    def length(self, back):
        return self.scorer.length(back, self.root)

    def pattern_lengths(self, back):
        if self.edge is None:
            return self.scorer.root_row(back, self.root)
        return self.scorer.edge_row(back, *self.edge)

    # -- saveCurrentTree with _pattern_pars = the booked tree's own row
    def book(self, length, kind, edge):
        if not self.bb:
            return
        self.edge = edge
        self.pattern_pars = self.pattern_lengths(self.back)
        self.rows.append((kind, edge, int(length), self.pattern_pars.copy(), list(self.back)))
        before = len(self.treels_logl)
        trees_before = list(self.boot_trees)
        self.save_current_tree(-float(length))
        self.took.append(sum(1 for a, b in zip(trees_before, self.boot_trees) if a != b))
        grew = len(self.treels_logl) > before
        if grew:
            self.kind_of[before] = kind
        self.calls.append((kind, self.step, before if grew else None))

    # -- the two questions SnkNniWitness.optimize asks
    def _current_length(self, back):
        self.cur = int(self.length(back))
        return self.cur

    def score_branch(self, v1, v2):
        if self.cur is not None:                      # the step's first branch: the current tree first (iqtree.cpp:2181-2183)
            self.step += 1
            self.book(self.cur, "cur", None)
            self.cur = None
        lens = []
        mvs = self.branch_moves(v1, v2)
        for mv in mvs:
            self.swap(mv, log=False)
            lens.append(self.scorer.edge_length(self.back, v1, v2))
            self.book(lens[-1], "cand", (v1, v2))     # phylotree.cpp:3937
            self.swap(mv, log=False)
        return lens[0], lens[1], mvs[0], mvs[1]

    def optimize_nni(self, speednni=True, max_steps=50):
        """-> (length, nni_count, nni_steps)"""
        self.log = []
        self.cur = None
        return SnkNniWitness.optimize(self, speednni, max_steps)

    # -- what the tests ask of a run
    def final_trees_booked_as_candidates(self):
        if self.mulhits:
            return sum(1 for s in self.boot_sets for t in s if self.kind_of.get(t) == "cand")
        return sum(1 for t in self.boot_trees if t >= 0 and self.kind_of.get(t) == "cand")

    def candidate_calls(self):
        """(accepted, rejected) by the cut-off among the candidates' saveCurrentTree calls"""
        acc = sum(1 for k, _s, t in self.calls if k == "cand" and t is not None)
        rej = sum(1 for k, _s, t in self.calls if k == "cand" and t is None)
        return acc, rej


def make(fx, cost, tie_seed, samples=None, root_taxon=1, weights=None):
    return SnkNniBbWitness(fx["codes_np"], fx["weights_np"] if weights is None else weights, fx["datatype"], cost, tie_seed, samples, root_taxon)
