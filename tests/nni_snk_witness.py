"""Witness of mpboot's NNI hill climb under a cost matrix (-cost m -nni_pars) -- TEST INFRASTRUCTURE ONLY.

Under -cost the search tree is a ParsTree (reference phyloanalysis.cpp:2200-2203, parstree.h:13), so IQTree::optimizeNNI scores
every NNI through ParsTree::computeParsimonyBranch (parstree.cpp:439-541) and the tree itself through ParsTree::computeParsimony
(:101-116).  The climb is NniWitness's (tests/nni_witness.py) with the one weighted-only rule, iqtree.cpp:2258: a step whose tree
came out longer than its best NNI promised is NOT rolled back -- the moves stay, the longer length stays, nni_count does not grow.

The scorer is a textbook Sankoff post-order dynamic programme over the record links back[], written for this file:
    view(rec)[i]   = cost of the subtree at node rec // 3 looking away from back[rec], that node in state i
                   = sum over its two children c of  min_j( view(c)[j] + cost[i][j] )          (a tip: 0 inside its state set)
    edge_length(node1, node2) = sum_ptn w * min_i( view(node2 side)[i] + min_j( view(node1 side)[j] + cost[i][j] ) )
the tree rooted at the branch with node2's side as the parent, the orientation of computeParsimonyBranch(node1->findNeighbor(node2),
node1); length(root tip) is the same at the root leaf's edge with the rest of the tree as the parent.  Views are remembered by the
shape of their subtree, so a swap recomputes only what it changes; nothing is taken from the engine or from oracle/.
"""
import sys

import numpy as np

from nni_witness import NniWitness, std_sort


def closed(cost):
    """the loader's triangle repair (parstree.cpp:74-80)"""
    c = np.array(cost, dtype=np.int64)
    for k in range(c.shape[0]):
        c = np.minimum(c, c[:, k:k + 1] + c[k:k + 1, :])
    return c


def tip_sets(codes, protein):
    """PLL tip codes -> state sets as bit masks: DNA codes are the masks; protein 0..19 one state, 20 = B (D or N), 21 = Z (Q or E),
    22 and above unknown"""
    c = np.asarray(codes, dtype=np.int64)
    if not protein:
        return c
    m = np.where(c < 20, 1 << np.minimum(c, 19), (1 << 20) - 1)
    m = np.where(c == 20, (1 << 2) | (1 << 3), m)
    return np.where(c == 21, (1 << 5) | (1 << 6), m)


class SnkScorer:
    def __init__(self, codes, weights, cost, protein=False):
        self.n, self.P = codes.shape
        self.S = 20 if protein else 4
        self.cost = closed(cost).astype(np.int32)          # (views are 32-bit like the engine's: lengths of these tests stay far below 2^31)
        assert self.cost.shape == (self.S, self.S)
        self.w = np.asarray(weights, dtype=np.int64)
        sets = tip_sets(codes, protein)
        big = int(self.cost.max()) + 1
        self.tips = [np.where((sets[t][None, :] >> np.arange(self.S)[:, None]) & 1, 0, big).astype(np.int32) for t in range(self.n)]
        self.shape_id = {}            # (child shape, child shape) -> shape number; tips are 1 .. n
        self.views = {}               # shape number -> (view, transform)
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 8 * self.n + 200))

    def transform(self, v):
        """m[i] = min_j( v[j] + cost[i][j] )"""
        return np.min(v[None, :, :] + self.cost[:, :, None], axis=1)

    def _shape(self, back, rec):
        node = rec // 3
        if node <= self.n:
            return node
        a = self._shape(back, int(back[3 * node + (rec + 1) % 3]))
        b = self._shape(back, int(back[3 * node + (rec + 2) % 3]))
        key = (a, b) if a < b else (b, a)
        sid = self.shape_id.get(key)
        if sid is None:
            sid = self.shape_id[key] = self.n + 1 + len(self.shape_id)
            self.views[sid] = None
        if self.views.get(sid) is None:
            v = self._pair(a)[1] + self._pair(b)[1]
            self.views[sid] = (v, self.transform(v))
        return sid

    def _pair(self, sid):
        if sid <= self.n:
            if sid not in self.views:
                self.views[sid] = (self.tips[sid - 1], self.transform(self.tips[sid - 1]))
        return self.views[sid]

    def view(self, back, rec):
        if len(self.views) * 8 * self.S * self.P > (1 << 28):        # (long climbs: start over rather than grow without bound)
            self.views.clear()
            self.shape_id.clear()
        return self._pair(self._shape(back, rec))

    def _across(self, parent, child_transform):
        ptn = np.min(parent + child_transform, axis=0)
        return int((ptn.astype(np.int64) * self.w).sum())

    def edge_length(self, back, node1, node2):
        r1 = next(3 * node1 + s for s in range(3 if node1 > self.n else 1) if int(back[3 * node1 + s]) // 3 == node2)
        r2 = int(back[r1])
        return self._across(self.view(back, r2)[0], self.view(back, r1)[1])

    def length(self, back, root_taxon=1):
        """ParsTree::computeParsimony at the root leaf"""
        return self._across(self.view(back, int(back[3 * root_taxon]))[0], self.view(back, 3 * root_taxon)[1])


class SnkNniWitness(NniWitness):
    def __init__(self, back, n, scorer, root_taxon=1):
        super().__init__(back, n, lambda b: scorer.length(b, root_taxon), root_taxon)
        self.scorer = scorer
        self.kept_worse = 0           # steps that took the `continue` of iqtree.cpp:2258
        self.most_applied = 0         # most NNIs applied in one step

    def score_branch(self, v1, v2):
        """(len0, len1, move0, move1): each move done, the tree scored at the branch (node2's side the parent), the move undone"""
        lens = []
        mvs = self.branch_moves(v1, v2)
        for mv in mvs:
            self.swap(mv, log=False)
            lens.append(self.scorer.edge_length(self.back, v1, v2))
            self.swap(mv, log=False)
        return lens[0], lens[1], mvs[0], mvs[1]

    def optimize(self, speednni=True, max_steps=50):
        """-> (length, nni_count, nni_steps); NniWitness.optimize without the rollback"""
        cur = int(self.score_fn(self.back))
        brans = {}
        count = 0
        step = 1
        while step <= max_steps:
            if speednni and brans:
                order = [brans[k] for k in sorted(brans)]
            else:
                order = self.full_order()
            plus = []
            for v1, v2 in order:
                l0, l1, m0, m1 = self.score_branch(v1, v2)
                ln, mv = (l0, m0) if l0 < l1 else (l1, m1)
                if ln < cur:
                    plus.append((ln, mv))
            std_sort(plus, lambda a, b: a[0] < b[0])
            if not plus:
                break
            chosen = []
            for ln, mv in plus:
                if all(mv[0] != c[1][0] and mv[2] != c[1][0] and mv[0] != c[1][2] and mv[2] != c[1][2] for c in chosen):
                    chosen.append((ln, mv))
            self.most_applied = max(self.most_applied, len(chosen))
            for _ln, mv in chosen:
                self.swap(mv)
            if speednni:
                brans = {}
                for _ln, (v1, _s1, v2, _s2) in chosen:
                    self._add(brans, v1, v2)
                    self._in_branches(brans, 2, v1, v2)
                    self._in_branches(brans, 2, v2, v1)
            cur = int(self.score_fn(self.back))
            if cur <= chosen[0][0]:
                count += len(chosen)
            else:
                self.kept_worse += 1          # iqtree.cpp:2258: `continue` -- nothing reverted, nothing counted
            step += 1
        return cur, count, step
