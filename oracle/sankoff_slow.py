"""Slow Sankoff dynamic programme on PLL tip codes (numpy over patterns) -- TEST INFRASTRUCTURE ONLY.

An independent second implementation (plain post-order DP from scratch for a given topology, the textbook
algorithm behind ParsTree::computePartialParsimony / computeParsimonyBranch, reference parstree.cpp:127-322,
:439-541) used to cross-check oracle/fitch_oracle.c's Sankoff mode and the weighted kernels.  Everything is int64 on the
data type's own states (binary 2, DNA 4, protein 20, multistate 32): no packing, no tiling, no padded states.
Parity status: UNPINNED against a reference run (sprparsimony.cpp / parstree.cpp cannot be built from their sources
alone).
"""
import sys

import numpy as np

DNA, AA, BIN, GENERIC = 0, 1, 2, 3
STATES = {DNA: 4, AA: 20, BIN: 2, GENERIC: 32}


def state_sets(codes, datatype):
    """PLL tip codes -> bit masks (pllrepo/src/globalVariables.h:60-78, :98-102): DNA and binary codes are the masks themselves,
    protein 0..19 one state each, 20 = B (N|D), 21 = Z (Q|E), 22 = any; multistate 0..31 one state each, 32 = any."""
    c = codes.astype(np.int64)
    if datatype in (DNA, BIN):
        return c
    if datatype == GENERIC:
        return np.where(c < 32, np.left_shift(1, np.minimum(c, 31)), (1 << 32) - 1)
    m = np.where(c < 20, np.left_shift(1, np.minimum(c, 19)), 0)
    m = np.where(c == 20, 12, m)
    m = np.where(c == 21, 96, m)
    m = np.where(c >= 22, (1 << 20) - 1, m)
    return m


def close_triangle(cost):
    c = np.array(cost, dtype=np.int64)
    S = c.shape[0]
    for k in range(S):
        for i in range(S):
            for j in range(S):
                if c[i, j] > c[i, k] + c[k, j]:
                    c[i, j] = c[i, k] + c[k, j]
    return c


def _nx(r):
    v, s = divmod(r, 3)
    return 3 * v + (s + 1) % 3


class _Views:
    """the directed views of one topology: down(rec) = cost rows [S][P] of the subtree behind record rec, seen from back[rec]"""

    def __init__(self, codes, back, cost, datatype):
        self.n, self.P = codes.shape
        self.S = STATES[datatype]
        self.cost = close_triangle(cost)
        assert self.cost.shape == (self.S, self.S)
        self.big = int(self.cost.max()) + 1          # highest_cost: what a state outside a tip's set costs
        self.sets = state_sets(codes, datatype)
        self.back = back
        self.memo = {}
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * self.n + 100))

    def tipvec(self, t):
        v = np.empty((self.S, self.P), dtype=np.int64)
        for k in range(self.S):
            v[k] = np.where((self.sets[t - 1] >> k) & 1, 0, self.big)
        return v

    def mplus(self, v):                # m[z] = min_x (v[x] + cost[z][x]): z the parent's state, x the child's
        return np.min(v[None, :, :] + self.cost[:, :, None], axis=1)

    def down(self, rec):
        if rec not in self.memo:
            if rec // 3 <= self.n:
                self.memo[rec] = self.tipvec(rec // 3)
            else:
                self.memo[rec] = self.mplus(self.down(int(self.back[_nx(rec)]))) + self.mplus(self.down(int(self.back[_nx(_nx(rec))])))
        return self.memo[rec]

    def at_branch(self, child):
        """per-pattern lengths rooted on the branch (child, back[child]): the subtree behind `child` is transformed, the rest of the
        tree is the parent side (the rows of the matrix): min_i(rest[i] + min_j(sub[j] + cost[i][j]))"""
        return np.min(self.down(int(self.back[child])) + self.mplus(self.down(child)), axis=0)


def tree_cost(codes, weights, back, cost, datatype=0, root_tip=1, root_rec=None):
    """-> (weighted tree cost, per-pattern costs) rooted on the branch of tip `root_tip`: min_i(rest[i] + min_j(leaf[j] + cost[i][j])),
    the rest of the tree as the parent side (ParsTree::computeParsimonyBranch, parstree.cpp:439-541, from computeParsimony :101-116).
    root_rec (instead of root_tip; matters for a matrix that is not symmetric only): root on the branch (root_rec, back[root_rec]) with
    the subtree behind root_rec in the leaf's place and everything behind back[root_rec] as the parent side."""
    v = _Views(codes, back, cost, datatype)
    ptn = v.at_branch(3 * root_tip if root_rec is None else int(root_rec))
    return int((ptn * np.asarray(weights, dtype=np.int64)).sum()), ptn


def largest_entries(codes, back, cost, datatype=0, moves=()):
    """-> (largest entry of any directed view of the tree or of any min-plus transform of one, largest per-state sum of three
    transforms that a candidate or an evaluation can form).  The tree itself and every tree apply_spr(back, p, q) for (p, q) in
    `moves` are walked, all 2 (2n - 3) directed views each.  Three transforms meeting at one point are at most three times the
    largest transform, and the sums actually formed -- m(a) + m(b) + m(c) at every inner node, before the minimum over states is
    taken -- are what the second number is taken over (with a tip's own row in the place of its transform where an evaluation reads
    it untransformed: never larger than highest_cost)."""
    top_view, top_sum = 0, 0
    for mv in (None,) + tuple(moves):
        b = back if mv is None else apply_spr(back, mv[0], mv[1])
        v = _Views(codes, b, cost, datatype)
        for node in range(1, 2 * v.n - 1):
            recs = [3 * node] if node <= v.n else [3 * node, 3 * node + 1, 3 * node + 2]
            for r in recs:
                d = v.down(r)
                top_view = max(top_view, int(d.max()), int(v.mplus(d).max()))
            if node > v.n:
                tot = sum(v.mplus(v.down(int(b[r]))) for r in recs)
                top_sum = max(top_sum, int(tot.max()))
            else:
                tot = v.down(int(b[3 * node])) + v.mplus(v.down(3 * node))
                top_sum = max(top_sum, int(tot.max()))
    return top_view, top_sum


def apply_spr(back, p, q):
    """prune node record p (with the subtree behind back[p]) and regraft it on branch (q, back[q])."""
    b = np.array(back, dtype=np.int32).copy()

    a1, a2 = int(b[_nx(p)]), int(b[_nx(_nx(p))])
    b[a1], b[a2] = a2, a1
    r = int(b[q])
    b[_nx(p)], b[q] = q, _nx(p)
    b[_nx(_nx(p))], b[r] = r, _nx(_nx(p))
    return b
