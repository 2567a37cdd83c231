"""Witness of mpboot's NNI hill climb under -bb (save_all_trees == 2) -- TEST INFRASTRUCTURE ONLY.

IQTree::optimizeNNI (reference iqtree.cpp:2173-2302) and getBestNNIForBran (phylotree.cpp:3807-3980) call saveCurrentTree

  1. at the start of every step that is not a rollback step (:2181-2183): the current tree with curScore;
  2. for every branch the step evaluates, in evaluation order, move 0 and then move 1 (phylotree.cpp:3907-3939): the swapped
     tree with the length optimizeOneBranch returned -- ALL evaluated moves, not only the positive ones;
  3. never in a rollback step, for the applied moves or for the rollback itself.

pllComputePatternParsimony is skipped on this path (iqtree.cpp:3363) and _pattern_pars is the booked tree's own row (for a
candidate computeParsimonyBranch has just written it, phylotree.cpp:956-957 / :986-987; for the current tree the last
whole-tree computeParsimony left it), so here `pattern_pars` is set to the booked tree's own per-pattern lengths BEFORE every
call: on a ratchet climb the length the cut-off test sees and treels_logl records is the booked tree's own length on the
original alignment.

The climb is the logic of tests/nni_witness.py:NniWitness (evaluation order, the std::sort port, the greedy choice, swaps,
rollback), the bookkeeping is oracle/search_slow.py:SlowSearch.save_current_tree; both are imported, nothing is copied.  Every
candidate is built (the swap done on back[]) and scored from scratch by SlowSearch.length; nothing is incremental.
SlowSearch.save_current_tree recomputes pattern_pars from self.back after the cut-off test: self.back holds the SWAPPED tree
during a candidate's call, so that gives the row it was handed.
"""
import numpy as np

from nni_witness import NniWitness, std_sort
from oracle.search_slow import SlowSearch


class NniBbWitness(SlowSearch, NniWitness):
    def __init__(self, codes, weights, datatype, informative, tie_seed, samples=None, root_taxon=1, eps=0.5):
        SlowSearch.__init__(self, codes, weights, datatype, informative, tie_seed, samples, eps)
        # SlowSearch knows the DNA and protein tip codes; binary data is coded like DNA (bitVectorIdentity) and 32-state data as
        # one bit per symbol with code 32 = every state (bitVector32, globalVariables.h:60-102)
        c = np.asarray(codes).astype(np.int64)
        if datatype == 2:
            self.sets = c
        elif datatype == 3:
            self.sets = np.where(c < 32, np.left_shift(1, np.minimum(c, 31)), (1 << 32) - 1)
        self.root = root_taxon
        self.log = []                                 # every swap of the last climb, reverts included
        self.rollbacks = 0
        self.calls = []                               # every saveCurrentTree call: (kind, step, booked index or None)
        self.kind_of = {}                             # tree index -> "cur" | "cand": what the tree booked under it was
        self.took = []                                # per call: how many samples' boot_trees entry the call changed

    # -- saveCurrentTree with _pattern_pars = the booked tree's own row
    def book(self, length, kind, step):
        if not self.bb:
            return
        self.pattern_pars = self.pattern_lengths(self.back)
        before = len(self.treels_logl)
        trees_before = list(self.boot_trees)
        self.save_current_tree(-float(length))
        self.took.append(sum(1 for a, b in zip(trees_before, self.boot_trees) if a != b))
        grew = len(self.treels_logl) > before
        if grew:
            self.kind_of[before] = kind
        self.calls.append((kind, step, before if grew else None))

    def optimize_nni(self, speednni=True, max_steps=50):
        """-> (length, nni_count, nni_steps)"""
        self.log = []
        cur = self.length(self.back)
        brans = {}
        rollback = False
        count = 0
        num = 0
        chosen = []
        step = 1
        while step <= max_steps:
            old = cur
            if not rollback:
                self.book(cur, "cur", step)                                  # iqtree.cpp:2181-2183
                if speednni and brans:
                    order = [brans[k] for k in sorted(brans)]
                else:
                    order = self.full_order()
                plus = []
                for v1, v2 in order:
                    lens = []
                    mvs = self.branch_moves(v1, v2)
                    for mv in mvs:
                        self.swap(mv, log=False)
                        lens.append(self.length(self.back))
                        self.book(lens[-1], "cand", step)                    # phylotree.cpp:3937
                        self.swap(mv, log=False)
                    ln, mv = (lens[0], mvs[0]) if lens[0] < lens[1] else (lens[1], mvs[1])
                    if ln < cur:
                        plus.append((ln, mv))
                std_sort(plus, lambda a, b: a[0] < b[0])
                if not plus:
                    break
                chosen = []
                for ln, mv in plus:
                    if all(mv[0] != c[1][0] and mv[2] != c[1][0] and mv[0] != c[1][2] and mv[2] != c[1][2] for c in chosen):
                        chosen.append((ln, mv))
                num = len(chosen)
            for i in range(num):
                self.swap(chosen[i][1])
            if speednni:
                brans = {}
                for i in range(num):
                    v1, _, v2, _ = chosen[i][1]
                    self._add(brans, v1, v2)
                    self._in_branches(brans, 2, v1, v2)
                    self._in_branches(brans, 2, v2, v1)
            cur = self.length(self.back)
            if cur <= chosen[0][0]:
                count += num
                rollback = False
            else:
                for i in range(num):
                    self.swap(chosen[i][1])
                rollback = True
                num = 1
                cur = old
                self.rollbacks += 1
            step += 1
        return cur, count, step

    # -- what the tests ask of a run
    def final_trees_booked_as_candidates(self):
        return sum(1 for t in self.boot_trees if t >= 0 and self.kind_of.get(t) == "cand")

    def candidate_calls(self):
        """(accepted, rejected) by the cut-off among the candidates' saveCurrentTree calls"""
        acc = sum(1 for k, _s, t in self.calls if k == "cand" and t is not None)
        rej = sum(1 for k, _s, t in self.calls if k == "cand" and t is None)
        return acc, rej


def make(fx, tie_seed, samples=None, root_taxon=1, keep_all=False, weights=None):
    inf = np.ones(len(fx["weights"]), dtype=bool) if keep_all else np.asarray(fx["informative"], dtype=bool)
    return NniBbWitness(fx["codes_np"], fx["weights_np"] if weights is None else weights, fx["datatype"], inf, tie_seed, samples, root_taxon)
