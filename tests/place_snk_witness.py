"""Witness of taxon insertion on the weighted (-cost) engine -- TEST INFRASTRUCTURE ONLY, pure numpy / Python, nothing taken from the
engine.

On a ParsTree, PhyloTree::addTaxonMPFast (phylotree.cpp:1322-1378) scores a test with computeParsimonyBranch(added_node->neighbors[0],
added_node), neighbors[0] being the new taxon: the FULL weighted length of the completed tree evaluated at the new taxon's edge,
the taxon the transformed side and the rest of the tree the rows of the matrix (parstree.cpp:439-541, the leaf swap at :449-457).
That is the completed tree's length at root leaf = the query.  With a matrix that is not symmetric the edge matters.

Forms, written differently on purpose:
  recursive_length   per pattern, plain Python integers: polytomy_witness._rec_snk (parstree.cpp:191-214 line by line) from the query
                     leaf, joined as polytomy_witness.recursive_weighted joins its root edge; tests/test_place_snk_witness.py shows
                     it IS recursive_weighted(..., root = query)[0].  Small cases only;
  SnkPlaceWitness.costs        the completed tree BUILT as an explicit adjacency map (place_witness.attached) and scored from scratch
                     by one recursive pass from the query leaf, numpy over the patterns -- no directed views, no join of two sides
                     (reuse=True: subtree rows met in an earlier completed tree of the same backbone come from a table);
  SnkPlaceWitness.view_costs   vectorised, on PolyWitness._views:  min_i( m(T_q)[i] + m(A_b)[i] + m(B_b)[i] ), for the larger cases.
stepwise mirrors place_witness.stepwise for computeParsimonyTree: lengths[0] = the star at leaf order[0], lengths[k - 2] = the score
addTaxonMPFast returned for order[k].
"""
import sys

import numpy as np

import place_witness as plw
import polytomy_witness as pw

STATES = {0: 4, 1: 20, 3: 32}


def recursive_length(codes, weights, datatype, cost, first, nbr, root):
    """the `length` of polytomy_witness.recursive_weighted(codes, weights, datatype, cost, first, nbr, root) without its branch
    substitutions: DNA and protein"""
    n, P = codes.shape
    S = 20 if datatype == 1 else 4
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 200))
    sets = pw.tip_sets(codes, datatype)
    c = [[int(x) for x in row] for row in pw.closed(cost)]
    big = max(max(row) for row in c) + 1
    r0 = pw._tip_neighbour(first, nbr, n, root)
    total = 0
    for p in range(P):
        tipcost = [[0 if (int(sets[t][p]) >> k) & 1 else big for k in range(S)] for t in range(n)]
        par, kid = pw._rec_snk(first, nbr, n, S, c, tipcost, r0, root), tipcost[root - 1]
        total += int(weights[p]) * min(par[i] + min(kid[j] + c[i][j] for j in range(S)) for i in range(S))
    return total


class _Views(pw.PolyWitness):
    """PolyWitness's weighted views for any alphabet of the weighted engine (PolyWitness itself knows 4 and 20 states)"""

    def __init__(self, codes, weights, datatype, cost):
        self.n, self.P = codes.shape
        self.S = STATES[datatype]
        self.w = np.asarray(weights, dtype=np.int64)
        self.keep = None
        self.sets = plw.tip_sets(codes, datatype)
        self.cost = pw.closed(cost)
        big = int(self.cost.max()) + 1
        # the narrowest integers that hold every sum formed here (three sides of a tree of n tips, one more matrix entry): exact
        top = (3 * self.n + 2) * big
        self.dtype = np.int16 if top < 2 ** 15 else (np.int32 if top < 2 ** 31 else np.int64)
        self.cost = self.cost.astype(self.dtype)
        self.tips = [np.where((self.sets[t][None, :] >> np.arange(self.S)[:, None]) & 1, 0, big).astype(self.dtype) for t in range(self.n)]

    def _transform(self, v):
        """m[z] = min_x( v[x] + cost[z][x] ), state by state (PolyWitness forms the S x S x P array at once)"""
        out = v[0][None, :] + self.cost[:, 0][:, None]
        for x in range(1, self.S):
            out = np.minimum(out, v[x][None, :] + self.cost[:, x][:, None])
        return out


class SnkPlaceWitness:
    def __init__(self, codes, weights, datatype, cost, keep=None):
        codes = np.asarray(codes)
        w = np.asarray(weights, dtype=np.int64)
        if keep is not None:
            w = w * (np.asarray(keep) != 0)
        cols = np.flatnonzero(w > 0)                         # (a pattern of weight 0 adds nothing to any length)
        self.n = codes.shape[0]
        self.v = _Views(codes[:, cols], w[cols], datatype, cost)
        self.w = self.v.w
        self.cost = self.v.cost
        self.S = self.v.S

        self._m = self.v._transform                          # (the viewer is the parent: the rows of the matrix)
        self.mtips = [self._m(t) for t in self.v.tips]       # a tip's own transform, formed once

    def length_at(self, adj, root, memo=None, alias=None):
        """the explicit tree adj scored from scratch at leaf `root`: min_i( rest[i] + m(root tip)[i] ), the rest the parent side.
        memo (costs(reuse=True)): the rows of a subtree (node, seen from), kept from one completed tree of a backbone to the next;
        alias names the two subtrees next to the new node by the backbone branch they hang on"""
        n = self.n

        def down(v, dad):                                    # the cost rows of the subtree at v seen from dad (parstree.cpp:191-214)
            key = None if memo is None else alias.get((v, dad), (v, dad))
            if key in (memo or ()):
                return memo[key]
            total = 0
            for u in adj[v]:
                if u != dad:
                    total = total + (self.mtips[u - 1] if u <= n else self._m(down(u, v)))
            if memo is not None and v != adj[root][0]:       # (the new node's own rows belong to one tree only)
                memo[key] = total
            return total

        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, 4 * len(adj) + 100))
        try:
            rest = down(adj[root][0], root)
        finally:
            sys.setrecursionlimit(old)
        return int(np.min(rest + self.mtips[root - 1], axis=0).astype(np.int64) @ self.w)

    def length(self, first, nbr, root):
        return self.length_at(plw.adjacency(first, nbr, self.n), root)

    def costs(self, first, nbr, queries, root, branches=None, reuse=False):
        """(branches, cost[Q][m]): every completed tree built and scored from scratch at the query's edge; branches: per query the
        indices to do (others -1).  reuse: the recursion over a completed tree takes the rows of a subtree it has met in an earlier
        completed tree of this call from a table (a subtree that does not hold the new node is the same subtree in both) -- still
        one recursive pass per explicit tree from the query leaf, for the backbones too large to score every tree in full"""
        adj = plw.adjacency(first, nbr, self.n)
        br = plw.walk(first, nbr, self.n, root)
        cost = -np.ones((len(queries), len(br)), dtype=np.int64)
        memo = {} if reuse else None
        for qi, q in enumerate(queries):
            for bi, (a, b) in enumerate(br):
                if branches is None or bi in branches[qi]:
                    done = plw.attached(adj, int(q), a, b)
                    new = done[int(q)][0]
                    cost[qi, bi] = self.length_at(done, int(q), memo, {(a, new): (a, b), (b, new): (b, a)} if reuse else None)
        return br, cost

    def place(self, first, nbr, queries, root):
        br, cost = self.costs(first, nbr, queries, root)
        at = [plw.first_min(row.tolist()) for row in cost]
        return at, [br[i] for i in at], [int(cost[q, i]) for q, i in enumerate(at)]

    def view_costs(self, first, nbr, queries, root):
        """-> (branches, cost[Q][m], the backbone's length at `root`) from the directed views of the backbone"""
        order, up, down = self.v._views(first, nbr, root)
        T = self.v._transform
        mt = np.stack([T(self.v.tips[int(q) - 1]) for q in queries]) if len(queries) else np.zeros((0, self.S, len(self.w)), dtype=self.v.dtype)
        cost = np.zeros((len(queries), len(order)), dtype=np.int64)
        for bi, (_dad, v) in enumerate(order):
            both = T(up[v]) + T(down[v])
            cost[:, bi] = np.min(mt + both[None, :, :], axis=1).astype(np.int64) @ self.w
        length = int(np.min(up[order[0][1]] + T(self.v.tips[root - 1]), axis=0).astype(np.int64) @ self.w)
        return order, cost, length


def stepwise(wit, order, scratch=True):
    """-> (first, nbr, lengths): the star of the first three, then every further taxon at the first minimum of its row; scratch:
    rows by the from-scratch form (else the vectorised one)"""
    n = wit.n
    first, nbr = [0, 3], [int(x) for x in order[:3]]
    lengths = [wit.length(first, nbr, int(order[0]))]
    for t in order[3:]:
        if scratch:
            br, cost = wit.costs(first, nbr, [int(t)], int(order[0]))
        else:
            br, cost, _ = wit.view_costs(first, nbr, [int(t)], int(order[0]))
        at = plw.first_min(cost[0].tolist())
        first, nbr = plw.grow(first, nbr, n, int(t), br[at][0], br[at][1])
        lengths.append(int(cost[0, at]))
    return first, nbr, lengths
