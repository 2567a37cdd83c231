"""Witness of taxon insertion -- TEST INFRASTRUCTURE ONLY, pure numpy, nothing taken from the engine or from oracle/.

The reference tries a new taxon on every branch of a tree (PhyloTree::addTaxonMPFast, phylotree.cpp:1322-1378): a pre-order walk
from the root leaf -- first (root leaf, its neighbour), then the other neighbours of every node in neighbors[] order --, the score of
a test being the Fitch length of the whole tree with the taxon in the middle of that branch, and the FIRST strictly smallest score
wins.  PhyloTree::computeParsimonyTree (phylotree.cpp:1243-1320) grows a tree that way in a my_random_shuffle order (tools.h:2107-2113).

The main form here shares no idea with the engine's kernel: the tree with the tip attached is BUILT, as an explicit adjacency map,
and scored from scratch by a recursive Fitch pass over state sets -- no directed views, no join of two sides.  A second, vectorised
form (view_costs) does use views and is there for the size pin; the tests show the two agree on the small cases.

A backbone is CSR neighbour lists (first, nbr): tips 1 .. n, inner node i = node n + 1 + i, neighbours in the host's order; tips may
be absent.
"""
import sys

import numpy as np


def tip_sets(codes, datatype):
    """PLL tip codes -> state sets as bit masks (0 DNA and 2 binary: the code is the mask; 1 protein: 0..19 one state, 20 = B,
    21 = Z, else all; 3 the 32-symbol alphabet: 1 << code, 32 and above all)"""
    c = np.asarray(codes, dtype=np.int64)
    if datatype in (0, 2):
        return c
    if datatype == 3:
        return np.where(c < 32, np.left_shift(1, np.minimum(c, 31)), (1 << 32) - 1)
    m = np.where(c < 20, np.left_shift(1, np.minimum(c, 19)), (1 << 20) - 1)
    m = np.where(c == 20, (1 << 2) | (1 << 3), m)
    return np.where(c == 21, (1 << 5) | (1 << 6), m)


# ---------------------------------------------------------------- explicit trees, scored from scratch
def adjacency(first, nbr, n):
    """{node: [neighbours]} of the lists, the tips that occur included"""
    adj = {}
    for i in range(len(first) - 1):
        v = n + 1 + i
        adj[v] = [int(u) for u in nbr[int(first[i]):int(first[i + 1])]]
        for u in adj[v]:
            if u <= n:
                adj[u] = [v]
    return adj


def attached(adj, tip, a, b):
    """a copy of the tree with `tip` hung on a new node in the middle of branch (a, b)"""
    out = {v: list(l) for v, l in adj.items()}
    new = max(out) + 1
    out[a][out[a].index(b)] = new
    out[b][out[b].index(a)] = new
    out[new] = [tip, a, b]
    out[tip] = [new]
    return out


def fitch_length(adj, sets, weights, n, root):
    """Fitch length of the explicit binary tree adj, all patterns at once: a recursive post-order from the leaf `root`"""
    w = np.asarray(weights, dtype=np.int64)
    total = [0]

    def down(v, dad):
        if v <= n:
            return sets[v - 1]
        kids = [u for u in adj[v] if u != dad]
        assert len(kids) == 2
        x, y = down(kids[0], v), down(kids[1], v)
        both = x & y
        total[0] += int(w[both == 0].sum())
        return np.where(both == 0, x | y, both)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * len(adj) + 100))
    try:
        rest = down(adj[root][0], root)
    finally:
        sys.setrecursionlimit(old)
    return total[0] + int(w[(rest & sets[root - 1]) == 0].sum())


# ---------------------------------------------------------------- the hand-over: check, walk, first minimum
def check(first, nbr, n, root):
    """'ok' | 'invalid' | 'unsupported' (a tree with an inner node of degree other than 3)"""
    first = [int(x) for x in first]
    nbr = [int(x) for x in nbr]
    k = len(first) - 1
    if not 1 <= k <= n - 2 or first[0] != 0 or not 1 <= root <= n or first[-1] > 3 * (n - 2) or first[-1] > len(nbr):
        return "invalid"
    N = n + k
    seen, arcs = set(), set()
    for i in range(k):
        lst = nbr[first[i]:first[i + 1]]
        if len(lst) < 3:
            return "invalid"
        for u in lst:
            if not 1 <= u <= N or u == n + 1 + i:
                return "invalid"
            if u <= n:
                if u in seen:
                    return "invalid"
                seen.add(u)
            elif (n + 1 + i, u) in arcs:
                return "invalid"
            else:
                arcs.add((n + 1 + i, u))
    m = len(seen)
    if m < 3 or root not in seen or any((b, a) not in arcs for a, b in arcs):
        return "invalid"
    if m + len(arcs) // 2 != m + k - 1:
        return "invalid"
    adj = adjacency(first, nbr, n)
    reach, st = {root}, [root]
    while st:
        v = st.pop()
        for u in adj[v]:
            if u not in reach:
                reach.add(u)
                st.append(u)
    if len(reach) != m + k:
        return "invalid"
    return "ok" if all(first[i + 1] - first[i] == 3 for i in range(k)) else "unsupported"


def walk(first, nbr, n, root):
    """the branches [(node1, node2)] in addTaxonMPFast's order, node1 the root side"""
    adj = adjacency(first, nbr, n)
    out, st = [], [(adj[root][0], root)]
    while st:
        v, dad = st.pop()
        out.append((dad, v))
        if v > n:
            st.extend((u, v) for u in reversed(adj[v]) if u != dad)
    return out


def first_min(row):
    best = 0
    for i, x in enumerate(row):
        if x < row[best]:
            best = i
    return best


class PlaceWitness:
    def __init__(self, codes, weights, datatype, keep=None):
        self.n = codes.shape[0]
        self.sets = tip_sets(codes, datatype).astype(np.uint8 if datatype in (0, 2) else np.int64)     # (DNA and binary sets fit a byte)
        self.w = np.asarray(weights, dtype=np.int64)
        if keep is not None:
            self.w = self.w * (np.asarray(keep) != 0)

    def length(self, first, nbr, root):
        return fitch_length(adjacency(first, nbr, self.n), self.sets, self.w, self.n, root)

    def costs(self, first, nbr, queries, root, branches=None):
        """(branches, cost[Q][m]): every tree-plus-taxon built and scored from scratch; branches: indices to do (others -1)"""
        adj = adjacency(first, nbr, self.n)
        br = walk(first, nbr, self.n, root)
        cost = -np.ones((len(queries), len(br)), dtype=np.int64)
        for qi, q in enumerate(queries):
            for bi, (a, b) in enumerate(br):
                if branches is None or bi in branches[qi]:
                    cost[qi, bi] = fitch_length(attached(adj, int(q), a, b), self.sets, self.w, self.n, root)
        return br, cost

    def place(self, first, nbr, queries, root):
        br, cost = self.costs(first, nbr, queries, root)
        at = [first_min(row.tolist()) for row in cost]
        return at, [br[i] for i in at], [int(cost[q, i]) for q, i in enumerate(at)]

    # ---- the vectorised, view-based form (size pin)
    def view_costs(self, first, nbr, queries, root):
        n = self.n
        adj = adjacency(first, nbr, n)
        br = walk(first, nbr, n, root)
        parent = {v: d for d, v in br}
        w = self.w

        def join(x, y):
            both = x & y
            return np.where(both == 0, x | y, both), int(w[both == 0].sum())

        up, down, length = {}, {}, 0
        for d, v in reversed(br):
            if v <= n:
                up[v] = self.sets[v - 1]
            else:
                a, b = [u for u in adj[v] if u != d]
                up[v], s = join(up[a], up[b])
                length += s
        length += join(self.sets[root - 1], up[br[0][1]])[1]
        down[br[0][1]] = self.sets[root - 1]
        for d, v in br:
            if v > n:
                a, b = [u for u in adj[v] if u != parent[v]]
                down[a] = join(down[v], up[b])[0]
                down[b] = join(down[v], up[a])[0]
        X = np.stack([join(down[v], up[v])[0] for _, v in br])                      # [m][P]
        cost = np.zeros((len(queries), len(br)), dtype=np.int64)
        for qi, q in enumerate(queries):
            cost[qi] = length + ((X & self.sets[int(q) - 1][None, :]) == 0).astype(np.int64) @ w
        return br, cost, length


# ---------------------------------------------------------------- computeParsimonyTree
def shuffle(n, lcg):
    """my_random_shuffle over the identity on an rng.Lcg64 stream: for i = n - 1 .. 1 swap(order[i], order[random_int(i + 1)])"""
    order = list(range(1, n + 1))
    r = lcg.doubles(n - 1)
    for j, i in enumerate(range(n - 1, 0, -1)):
        k = int(np.floor(r[j] * (i + 1)))
        order[i], order[k] = order[k], order[i]
    return order


def grow(first, nbr, n, tip, node1, node2):
    """the reference's rewiring: the new inner node replaces target_dad (node1) in target_node's (node2's) list and the other way
    round, in place, and lists [tip, target_node, target_dad]"""
    first = [int(x) for x in first]
    nbr = [int(x) for x in nbr]
    new = n + len(first)
    lists = [nbr[first[i]:first[i + 1]] for i in range(len(first) - 1)]
    if node2 > n:
        l = lists[node2 - n - 1]
        l[l.index(node1)] = new
    if node1 > n:
        l = lists[node1 - n - 1]
        l[l.index(node2)] = new
    lists.append([tip, node2, node1])
    return list(np.cumsum([0] + [len(l) for l in lists])), [u for l in lists for u in l]


def stepwise(wit, order):
    """-> (first, nbr, lengths): lengths[j] = the length of the tree of the first j + 3 taxa"""
    n = wit.n
    first, nbr = [0, 3], [int(x) for x in order[:3]]
    lengths = [wit.length(first, nbr, int(order[0]))]
    for t in order[3:]:
        _at, brs, ln = wit.place(first, nbr, [int(t)], int(order[0]))
        first, nbr = grow(first, nbr, n, int(t), brs[0][0], brs[0][1])
        lengths.append(ln[0])
    return first, nbr, lengths


# ---------------------------------------------------------------- malformed hand-overs (n = 9; the good one has tips 1 .. 7)
def backbone(n, tips, rng):
    """a random binary backbone over `tips`, grown by attaching each to a random branch"""
    tips = [int(t) for t in tips]
    first, nbr = [0, 3], tips[:3]
    for t in tips[3:]:
        br = walk(first, nbr, n, tips[0])
        a, b = br[int(rng.integers(len(br)))]
        first, nbr = grow(first, nbr, n, t, a, b)
    return np.array(first, dtype=np.int32), np.array(nbr, dtype=np.int32)


GOOD = ([0, 3, 6, 9], [1, 2, 11, 10, 3, 12, 11, 4, 5])                   # ((1,2),3,(4,5)) over n = 9: tips 6 .. 9 absent
MALFORMED = {
    "tip twice": ([0, 3, 6, 9], [1, 2, 11, 10, 3, 12, 11, 4, 1], 1, "invalid"),
    "degree 4": ([0, 3, 7], [1, 2, 11, 10, 3, 4, 5], 1, "unsupported"),
    "cycle": ([0, 3, 6, 9], [1, 11, 12, 10, 12, 2, 10, 11, 3], 1, "invalid"),
    "disconnected": ([0, 3, 6, 9, 12], [1, 2, 11, 10, 3, 4, 13, 5, 6, 12, 7, 8], 1, "invalid"),
    "root absent": ([0, 3, 6, 9], [1, 2, 11, 10, 3, 12, 11, 4, 5], 7, "invalid"),
    "two tips": ([0, 3], [1, 2, 10], 1, "invalid"),
}
