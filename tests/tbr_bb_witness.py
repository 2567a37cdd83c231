"""Witness of the TBR sweep and climb under -bb -- TEST INFRASTRUCTURE ONLY.

There is no reference function (MPBoot has SPR and NNI only), so the engine's header states the semantics and this file restates
them from scratch: a tracked sweep hands EVERY entry of every visit's matrix to IQTree::saveCurrentTree -- the visits in
node_order(), a visit's entries in row-major order from [0][0]; [0][0] is the current tree under its own length (as
rearrangeParsimony opens every prune node with a booking of the current tree), every other entry the joined tree; a 1 x 1 visit
books the current tree only.  Duplicated topologies are booked as often as they occur.

The enumeration is tests/tbr_witness.py's (lists, node_order, first_min; TbrWitness.descent is inherited as it stands and only the
sweep under it is replaced), the bookkeeping is oracle/search_slow.py:SlowSearch.save_current_tree; both are imported, nothing is
copied.  Every entry's tree is built (trees.apply_tbr) and scored from scratch by SlowSearch.length; nothing is incremental, no
root set and no mask is formed here.  SlowSearch.save_current_tree recomputes pattern_pars from self.back behind the cut-off test:
self.back holds the JOINED tree during an entry's call.
"""
import numpy as np

from mpboot_amd import trees
from oracle.search_slow import SlowSearch
from tbr_witness import NONE, NO_BEST, TbrWitness, first_min, lists, node_order


class TbrBbWitness(SlowSearch, TbrWitness):
    def __init__(self, codes, weights, datatype, informative, tie_seed, samples=None, eps=0.5):
        SlowSearch.__init__(self, codes, weights, datatype, informative, tie_seed, samples, eps)
        # SlowSearch knows the DNA and protein tip codes; 32-state data is one bit per symbol with code 32 = every state
        c = np.asarray(codes).astype(np.int64)
        if datatype == 2:
            self.sets = c
        elif datatype == 3:
            self.sets = np.where(c < 32, np.left_shift(1, np.minimum(c, 31)), (1 << 32) - 1)
        self.calls = []                               # every saveCurrentTree call: (kind, (visit, i, j), booked index or None)
        self.kind_of = {}                             # tree index -> (kind, i, j) of the entry booked under it
        self.took = []                                # per call: how many samples' boot_trees entry the call changed
        self.moves = []

    def length(self, back):                           # (SlowSearch's: from scratch, dropped patterns count nothing)
        return SlowSearch.length(self, back)

    def book_entry(self, length, kind, where):
        if not self.bb:
            return
        before = len(self.treels_logl)
        trees_before = list(self.boot_trees)
        self.save_current_tree(-float(length))
        self.took.append(sum(1 for a, b in zip(trees_before, self.boot_trees) if a != b))
        grew = len(self.treels_logl) > before
        if grew:
            self.kind_of[before] = (kind, where[1], where[2])
        self.calls.append((kind, where, before if grew else None))

    # what TbrWitness.descent asks of a sweep, every entry built, scored from scratch and booked on the way
    def sweep_best(self, back, maxtrav, spr_only=False):
        assert not spr_only
        back = np.array(back, dtype=np.int32)
        out, pairs = [], 0
        for v, p in enumerate(node_order(back, self.n)):
            F, G = lists(back, self.n, p, maxtrav)
            fr, gr = [NONE] + [r for r, _ in F], [NONE] + [r for r, _ in G]
            cost = np.empty((len(fr), len(gr)), dtype=np.int64)
            for i, f in enumerate(fr):
                for j, g in enumerate(gr):
                    self.back = [int(x) for x in trees.apply_tbr(back, p, f, g)]
                    cost[i, j] = SlowSearch.length(self, self.back)
                    self.book_entry(int(cost[i, j]), "cur" if i == 0 and j == 0 else "cand", (v, i, j))
            pairs += cost.size
            best = first_min(cost)
            out.append((NO_BEST, NONE, NONE) if best is None else (best[0], fr[best[1]], gr[best[2]]))
        self.back = [int(x) for x in back]
        return out, pairs

    def tbr_sweep(self, maxtrav):
        """-> ([(cost, f, g)] per visit, entries); the tree stays"""
        return self.sweep_best(self.back, maxtrav)

    def optimize_tbr(self, maxtrav, max_moves=0):
        """-> (length, n_moves); the moves in self.moves, the final tree in self.back"""
        back, length, moves = self.descent(self.back, maxtrav, max_moves)
        self.back = [int(x) for x in back]
        self.moves = moves
        return length, len(moves)

    # -- what the tests ask of a run
    def final_trees_booked_as_interior(self):
        """samples whose final boot tree was booked as an entry with i >= 1 and j >= 1"""
        def interior(t):
            k = self.kind_of.get(t)
            return k is not None and k[1] >= 1 and k[2] >= 1
        if self.mulhits:
            return sum(1 for s in self.boot_sets if any(interior(t) for t in s))
        return sum(1 for t in self.boot_trees if t >= 0 and interior(t))

    def candidate_calls(self):
        """(accepted, rejected) by the cut-off among the candidates' saveCurrentTree calls"""
        acc = sum(1 for k, _w, t in self.calls if k == "cand" and t is not None)
        rej = sum(1 for k, _w, t in self.calls if k == "cand" and t is None)
        return acc, rej
