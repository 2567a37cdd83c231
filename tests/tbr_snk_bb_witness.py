"""Witness of the TBR sweep and climb under -bb on the weighted (-cost) engine -- TEST INFRASTRUCTURE ONLY.

There is no reference function; the engine's header states the semantics (tests/tbr_bb_witness.py restates them for the Fitch engine)
and this file restates them for a cost matrix: a tracked sweep hands EVERY entry of every visit's matrix to IQTree::saveCurrentTree --
the visits in node_order(), a visit's entries in row-major order from [0][0]; [0][0] is the current tree under its own length, every
other entry the joined tree under its full weighted length; a 1 x 1 visit books the current tree only.  Duplicated topologies are
booked as often as they occur.  _pattern_pars of a booked tree is the row of per-pattern minima whose weighted sum its length is.

Nothing is copied.  The enumeration is tests/tbr_witness.py's (lists, node_order, first_min, TbrWitness.descent through
TbrBbWitness), the bookkeeping is oracle/search_slow.py:SlowSearch.save_current_tree (through TbrBbWitness.book_entry), and an
entry's length and row come from TbrSnkWitness's from-scratch form (a): the joined tree is built (trees.apply_tbr) and scored by one
recursive Sankoff pass from a root leaf.  Form (a) ends in `row @ weights`; the row is taken where that product is formed (a weight
vector that remembers its left operand), so length and row are the two halves of one evaluation.  No directed view, no chain and
no root set is formed here.  Symmetric cost matrices only, as on the engine: the row does not depend on the root leaf then
(tests/test_tbr_snk_bb_witness.py pins it at three leaves).
"""
import numpy as np

from mpboot_amd import trees
from tbr_bb_witness import TbrBbWitness
from tbr_snk_witness import TbrSnkWitness
from tbr_witness import NONE, NO_BEST, first_min, lists, node_order


class _Tap:
    """the weights of TbrSnkWitness.length, remembering the row they were last multiplied with"""
    __array_ufunc__ = None                            # ndarray @ _Tap defers to __rmatmul__

    def __init__(self, w):
        self.w, self.row = np.asarray(w, dtype=np.int64), None

    def __rmatmul__(self, row):
        self.row = np.array(row, dtype=np.int64)
        return self.row @ self.w


class RowScorer(TbrSnkWitness):
    """form (a) with the row behind its length"""

    def __init__(self, codes, weights, datatype, cost):
        TbrSnkWitness.__init__(self, codes, weights, datatype, cost)
        self.P = np.asarray(codes).shape[1]
        self.cols = np.flatnonzero(np.asarray(weights, dtype=np.int64) > 0)      # (the patterns TbrSnkWitness keeps)
        self.w = _Tap(self.w)

    def length_and_row(self, back, root=1, memo=None):
        """(weighted length, per-pattern lengths over ALL patterns, 0 at a pattern of weight 0) of the tree, from the leaf `root`"""
        total = TbrSnkWitness.length(self, back, root, memo)
        row = np.zeros(self.P, dtype=np.int64)
        row[self.cols] = self.w.row
        return total, row


class TbrSnkBbWitness(TbrBbWitness):
    def __init__(self, codes, weights, datatype, cost, tie_seed, samples=None, eps=0.5):
        TbrBbWitness.__init__(self, codes, weights, datatype, np.ones(np.asarray(codes).shape[1], dtype=bool), tie_seed, samples, eps)
        self.scorer = RowScorer(codes, weights, datatype, cost)
        self.memo = {}                                # subtree rows kept from one edited tree to the next (root leaf 1)
        self.rows = []                                # per saveCurrentTree call that booked: ((visit, i, j), length, row)

    # -- SlowSearch's two scoring entry points on form (a)
    def length(self, back):
        return self.scorer.length_and_row(back, 1, self.memo)[0]

    def pattern_lengths(self, back):
        return self.scorer.length_and_row(back, 1, self.memo)[1]

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
                    cost[i, j] = self.length(self.back)
                    before = len(self.treels_logl) if self.bb else 0
                    self.book_entry(int(cost[i, j]), "cur" if i == 0 and j == 0 else "cand", (v, i, j))
                    if self.bb and len(self.treels_logl) > before:
                        self.rows.append(((v, i, j), int(cost[i, j]), self.pattern_pars.copy()))
            pairs += cost.size
            best = first_min(cost)
            out.append((NO_BEST, NONE, NONE) if best is None else (best[0], fr[best[1]], gr[best[2]]))
        self.back = [int(x) for x in back]
        return out, pairs
