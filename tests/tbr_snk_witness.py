"""Witness of the TBR neighbourhood on the weighted (-cost) engine -- TEST INFRASTRUCTURE ONLY, pure numpy / Python, nothing taken
from the engine.

There is no reference function (MPBoot has SPR and NNI only).  The lists, the visiting order and the first-minimum rule are those
of tests/tbr_witness.py: they follow from back[] alone.  An entry is the FULL weighted length of the tree that joins the middle of
F[i - 1] to the middle of G[j - 1]; there is no additive base.  Symmetric cost matrices only: with any other the length depends on
the edge it is evaluated at (tests/test_tbr_snk_witness.py pins a seed that shows it), and TBR has no reference that would fix one.

Three forms, written differently on purpose:
  (a) from scratch: the edited tree is built (trees.apply_tbr) and scored by one recursive Sankoff pass from a root leaf, cost rows
      per subtree, no directed views;
  (b) vectorised: memoised directed views with their transforms, the chain MU of a side, the root sets (a side of G transformed),
      one min-plus product per visit -- the identity the engine rests on;
  (c) the enumeration, the per-visit first minimum, the sweep's best and steepest descent, as tbr_witness.TbrWitness has them.
"""
import sys

import numpy as np

import tbr_witness as tw
from mpboot_amd import trees
from place_witness import tip_sets
from polytomy_witness import closed

NONE = tw.NONE
NO_BEST = tw.NO_BEST
STATES = {0: 4, 1: 20, 3: 32}


def _deep(n):
    return max(sys.getrecursionlimit(), 8 * n + 200)


class TbrSnkWitness:
    def __init__(self, codes, weights, datatype, cost, keep=None):
        codes = np.asarray(codes)
        w = np.asarray(weights, dtype=np.int64)
        if keep is not None:
            w = w * (np.asarray(keep) != 0)
        cols = np.flatnonzero(w > 0)                         # (a pattern of weight 0 adds nothing to any length)
        self.n = codes.shape[0]
        self.S = STATES[datatype]
        self.w = w[cols]
        self.cost = closed(cost)
        assert self.cost.shape == (self.S, self.S)
        big = int(self.cost.max()) + 1                       # what a state outside a tip's set costs
        # the narrowest integers that hold every sum formed here: a vector, a transform or a root set stays within the tips behind it
        # times big (m(v)[z] <= v[z]), two sides hold n tips together, and a transform adds one more matrix entry before its minimum
        top = (self.n + 2) * big
        self.dtype = np.int16 if top < 2 ** 15 else (np.int32 if top < 2 ** 31 else np.int64)
        self.cost = self.cost.astype(self.dtype)
        sets = tip_sets(codes[:, cols], datatype)
        self.tips = [np.where((sets[t][None, :] >> np.arange(self.S)[:, None]) & 1, 0, big).astype(self.dtype) for t in range(self.n)]

    def m(self, v):
        """m[z] = min_x( v[x] + cost[z][x] ): the viewer is the parent, the rows of the matrix"""
        return np.min(v[None, :, :] + self.cost[:, :, None], axis=1)

    # ------------------------------------------------------------ (a) from scratch
    def length(self, back, root=1, memo=None):
        """the weighted length by a plain post-order recursion from the leaf `root`: min_x( rest[x] + m(leaf)[x] ).
        memo (a dict kept by the caller from one tree to the next; root 1 only): the cost rows of a subtree are taken from a table
        where the same subtree -- the same tips joined in the same shape -- was met before.  An edited tree shares all but a few
        subtrees with the tree it was made from; the pass over it is still one recursion from the root leaf over the explicit tree"""
        n = self.n
        table = {"ids": {}, "kids": {}, "rows": {}} if memo is None else memo
        if not table:
            table.update(ids={}, kids={}, rows={})
        ids, kids, done = table["ids"], table["kids"], table["rows"]

        def ident(r):                                        # a number for the subtree behind record r: equal subtrees, equal numbers
            if r // 3 <= n:
                return r // 3
            a, b = ident(int(back[tw.nx(r)])), ident(int(back[tw.nx(tw.nx(r))]))
            key = (min(a, b), max(a, b))
            if key not in ids:
                ids[key] = n + 1 + len(ids)
                kids[ids[key]] = key
            return ids[key]

        def rows_of(i):                                      # the cost rows of subtree i
            if i <= n:
                return self.tips[i - 1]
            if i not in done:
                total = 0
                for c in kids[i]:
                    rows = rows_of(c)
                    step = rows[0][None, :] + self.cost[:, 0][:, None]       # (state by state: m() forms the S x S x P array at once)
                    for x in range(1, self.S):
                        step = np.minimum(step, rows[x][None, :] + self.cost[:, x][:, None])
                    total = total + step
                done[i] = total
            return done[i]

        assert memo is None or root == 1
        old = sys.getrecursionlimit()
        sys.setrecursionlimit(_deep(n))
        try:
            rest = rows_of(ident(int(back[3 * root])))
        finally:
            sys.setrecursionlimit(old)
        leaf = self.tips[root - 1]
        across = np.min(leaf[None, :, :] + self.cost[:, :, None], axis=1)
        return int(np.min(rest + across, axis=0).astype(np.int64) @ self.w)

    def scratch(self, back, p, f, g, memo=None):
        return self.length(trees.apply_tbr(back, p, f, g), memo=memo)

    def scratch_matrix(self, back, p, maxtrav):
        F, G = tw.lists(back, self.n, p, maxtrav)
        fr, gr = [NONE] + [r for r, _ in F], [NONE] + [r for r, _ in G]
        return np.array([[self.scratch(back, p, f, g) for g in gr] for f in fr], dtype=np.int64)

    # ------------------------------------------------------------ (b) views, chains, root sets
    def views(self, back):
        """{record: (vector, its transform)}: what is seen behind every record of the tree"""
        n, memo = self.n, {}

        def view(r):
            if r not in memo:
                if r // 3 <= n:
                    v = self.tips[r // 3 - 1]
                else:
                    v = view(int(back[tw.nx(r)]))[1] + view(int(back[tw.nx(tw.nx(r))]))[1]
                memo[r] = (v, self.m(v))
            return memo[r]

        old = sys.getrecursionlimit()
        sys.setrecursionlimit(_deep(n))
        try:
            for v in range(1, 2 * n - 1):
                for s in range(1 if v <= n else 3):
                    view(3 * v + s)
        finally:
            sys.setrecursionlimit(old)
        return memo

    def root_sets(self, back, views, x, maxtrav):
        """[R(.)] along side_list(x): MU(child) = m( MU(parent) + m(vec[sibling]) ), R(g) = MU(g) + m(vec[g])"""
        n, out = self.n, []
        if x // 3 <= n or maxtrav < 1:
            return out
        x1, x2 = int(back[tw.nx(x)]), int(back[tw.nx(tw.nx(x))])
        if x1 // 3 <= n and x2 // 3 <= n:
            return out
        if ("part", x, maxtrav) in views:                    # (a part is F of one visit and G of the visit from the edge's other end)
            return views["part", x, maxtrav]

        def walk(q, sib, mup, d):
            mu = self.m(mup + views[sib][1])
            out.append(mu + views[q][1])
            if q // 3 > n and d < maxtrav:
                c1, c2 = int(back[tw.nx(q)]), int(back[tw.nx(tw.nx(q))])
                walk(c1, c2, mu, d + 1)
                walk(c2, c1, mu, d + 1)

        old = sys.getrecursionlimit()
        sys.setrecursionlimit(_deep(n))
        try:
            for a, other in ((x1, x2), (x2, x1)):
                if a // 3 > n:
                    c1, c2 = int(back[tw.nx(a)]), int(back[tw.nx(tw.nx(a))])
                    walk(c1, c2, views[other][1], 1)
                    walk(c2, c1, views[other][1], 1)
        finally:
            sys.setrecursionlimit(old)
        views["part", x, maxtrav] = out
        return out

    def matrix(self, back, p, maxtrav, views=None):
        """(F records, G records, cost[1 + |F|][1 + |G|]) by the identity: sum_ptn w * min_x( RF_i[x] + m(RG_j)[x] )"""
        views = views or self.views(back)
        q = int(back[p])
        F, G = tw.lists(back, self.n, p, maxtrav)
        rf = np.stack([views[q][0]] + self.root_sets(back, views, q, maxtrav))
        if ("moved", p, maxtrav) not in views:
            views["moved", p, maxtrav] = [self.m(r) for r in self.root_sets(back, views, p, maxtrav)]
        mrg = np.stack([views[p][1]] + views["moved", p, maxtrav])
        assert len(rf) == 1 + len(F) and len(mrg) == 1 + len(G)
        cost = np.empty((len(rf), len(mrg)), dtype=np.int64)
        for i in range(len(rf)):
            cost[i] = np.min(rf[i][None, :, :] + mrg, axis=1).astype(np.int64) @ self.w
        return [r for r, _ in F], [r for r, _ in G], cost

    # ------------------------------------------------------------ (c) sweep and descent
    def sweep_best(self, back, maxtrav, spr_only=False):
        """per visit of node_order: (cost, f, g) of its first minimum, or (NO_BEST, -1, -1); and the number of entries"""
        views, out, pairs = self.views(back), [], 0
        for p in tw.node_order(back, self.n):
            F, G, cost = self.matrix(back, p, maxtrav, views)
            pairs += cost.size
            if spr_only:
                cost = cost.copy()
                cost[1:, 1:] = np.iinfo(np.int64).max
            best = tw.first_min(cost)
            out.append((NO_BEST, NONE, NONE) if best is None else (best[0], ([NONE] + F)[best[1]], ([NONE] + G)[best[2]]))
        return out, pairs

    def descent(self, back, maxtrav, max_moves=0, spr_only=False):
        """steepest descent: the sweep's lowest cost (lowest visit among equals) while strictly below the current length
        -> (back, length, [(rec, f, g, length)])"""
        back = np.array(back, dtype=np.int32).copy()
        length, moves = self.length(back), []
        while not (max_moves > 0 and len(moves) >= max_moves):
            best, _ = self.sweep_best(back, maxtrav, spr_only)
            order = tw.node_order(back, self.n)
            at = min(range(len(best)), key=lambda i: (best[i][0], i))
            if best[at][0] == NO_BEST or best[at][0] >= length:
                break
            length = best[at][0]
            back = trees.apply_tbr(back, order[at], best[at][1], best[at][2])
            moves.append((order[at], best[at][1], best[at][2], length))
        return back, length, moves


# the input that shows TBR adds something on the weighted engine too: from the SPR-local optimum the restricted descent reaches at
# radius PINNED_RADIUS under tstv, the unrestricted descent finds a strictly shorter tree (found by a search over seeds on the CPU;
# tests/test_tbr_snk_witness.py checks it)
PINNED_SEED, PINNED_RADIUS = 6, 3
# under nni_snk_cases.asym(4, ASYM_SEED) the lengths of one tree at its root leaves differ: why such an engine is refused
ASYM_SEED = 4


def noisy_case(seed, n=12, P=120):
    """(codes, weights, start tree): random DNA patterns, nothing tree-like in them"""
    codes, weights = tw.alignment(n, P, "dna", 7000 + seed)
    return codes, weights, trees.random_topology(n, np.random.default_rng(9000 + seed))
