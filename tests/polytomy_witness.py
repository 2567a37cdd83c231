"""Witnesses of the reference's parsimony rules on MULTIFURCATING trees -- TEST INFRASTRUCTURE ONLY.

A tree is CSR neighbour lists (first, nbr): tips are nodes 1 .. n, inner node i (0-based) is node n + 1 + i with the neighbours
nbr[first[i]:first[i + 1]] in the host's neighbors[] order.  The rules at a node of any degree:

  * Fitch (PhyloTree::computePartialParsimony, generic path, reference phylotree.cpp:869-931): the set of a node is the AND of all
    its children's sets; where that is empty it is the OR of all of them and ONE step is counted -- one per node, whatever the
    degree.  Not the length of a hard polytomy, and it depends on the root leaf; it is what the reference prints;
  * weighted (ParsTree::computePartialParsimony, parstree.cpp:191-214): the cost row of a node is the sum over all children of
    min_j(child[j] + cost[i][j]);
  * the tree is evaluated at the root leaf: computeParsimonyBranch(root->neighbors[0], root) (phylotree.cpp:938-1047,
    parstree.cpp:439-541), and fixNegativeBranch (phylotree.cpp:3597-3633) walks it in pre-order from that leaf, neighbours in list
    order, and asks every branch for its branch_subst.

No is_const skip is applied (phylotree.cpp:845, :900; parstree.cpp:196): every pattern handed in takes the rule.

Two witnesses, written differently on purpose:
  PolyWitness          numpy over all patterns at once; the views away from the root in one post-order pass, the views towards it
                       in one pre-order pass that forms "all inputs but one" from prefix and suffix accumulations;
  recursive_*          per pattern, recursive, plain Python integers, restating the two reference loops line by line; the side of a
                       branch towards the root is got by re-rooting the recursion at the branch, no second pass at all.
Nothing is taken from the engine or from oracle/.
"""
import sys

import numpy as np


def tip_sets(codes, datatype):
    """PLL tip codes -> state sets as bit masks (0 DNA: the code is the mask; 1 protein: 0..19 one state, 20 = B, 21 = Z, else all)"""
    c = np.asarray(codes, dtype=np.int64)
    if datatype == 0:
        return c
    m = np.where(c < 20, np.left_shift(1, np.minimum(c, 19)), (1 << 20) - 1)
    m = np.where(c == 20, (1 << 2) | (1 << 3), m)
    return np.where(c == 21, (1 << 5) | (1 << 6), m)


def closed(cost):
    """the loader's triangle repair (parstree.cpp:74-80)"""
    c = np.array(cost, dtype=np.int64)
    for k in range(c.shape[0]):
        c = np.minimum(c, c[:, k:k + 1] + c[k:k + 1, :])
    return c


def neighbours(first, nbr, n, v):
    if v <= n:
        raise ValueError("a tip's neighbour is found through the lists")
    i = v - n - 1
    return [int(u) for u in nbr[int(first[i]):int(first[i + 1])]]


def validate(first, nbr, n):
    """None for a tree the hand-over accepts, else the reason (the checks of include/mpfitch.h, restated)"""
    first = [int(x) for x in first]
    k = len(first) - 1
    if not 1 <= k <= n - 2 or first[0] != 0:
        return "n_inner"
    N = n + k
    seen_tip = [0] * (n + 1)
    arcs = set()
    for i in range(k):
        lst = [int(u) for u in nbr[first[i]:first[i + 1]]]
        if len(lst) < 3:
            return "degree"
        for u in lst:
            if not 1 <= u <= N or u == n + 1 + i:
                return "range"
            if u <= n:
                seen_tip[u] += 1
            else:
                if (n + 1 + i, u) in arcs:
                    return "twice"
                arcs.add((n + 1 + i, u))
    if any(c != 1 for c in seen_tip[1:]):
        return "tips"
    if any((b, a) not in arcs for a, b in arcs):
        return "symmetry"
    if n + len(arcs) // 2 != N - 1:
        return "edges"
    reach, st = {n + 1}, [n + 1]
    while st:
        v = st.pop()
        for u in neighbours(first, nbr, n, v):
            if u > n and u not in reach:
                reach.add(u)
                st.append(u)
    return None if len(reach) == k else "connected"


def rooted(first, nbr, n, root):
    """-> (branches [(node1, node2)] in fixNegativeBranch's order, parent {node: dad})"""
    r0 = next(n + 1 + i for i in range(len(first) - 1) if root in neighbours(first, nbr, n, n + 1 + i))
    order, parent, st = [], {root: 0}, [(r0, root)]
    while st:
        v, dad = st.pop()
        parent[v] = dad
        order.append((dad, v))
        if v > n:
            st.extend((u, v) for u in reversed(neighbours(first, nbr, n, v)) if u != dad)
    return order, parent


def branch_lengths(subst, n_sites, n_states):
    """phylotree.cpp:3608-3614 in double precision"""
    s = np.asarray(subst, dtype=np.float64)
    N = np.float64(n_sites)
    bl = np.where(s > 0, s / N, np.float64(1.0) / N)
    z = np.float64(n_states) / np.float64(n_states - 1)
    x = np.float64(1.0) - z * bl
    with np.errstate(invalid="ignore", divide="ignore"):
        bl = np.where(x > 0, -np.log(np.where(x > 0, x, 1.0)) / z, bl)
    return np.maximum(bl, 1e-6)


class PolyWitness:
    """both rules, all patterns at once.  cost=None: Fitch; else the weighted rule under closed(cost)"""

    def __init__(self, codes, weights, datatype, cost=None, keep=None):
        self.n, self.P = codes.shape
        self.S = 20 if datatype == 1 else 4
        self.w = np.asarray(weights, dtype=np.int64)
        if keep is not None:
            self.w = self.w * (np.asarray(keep) != 0)
        self.keep = None if keep is None else (np.asarray(keep) != 0)
        self.sets = tip_sets(codes, datatype)
        self.cost = None if cost is None else closed(cost)
        if cost is not None:
            big = int(self.cost.max()) + 1
            self.tips = [np.where((self.sets[t][None, :] >> np.arange(self.S)[:, None]) & 1, 0, big).astype(np.int64) for t in range(self.n)]

    # ---- the rule over a list of inputs
    def _fitch(self, ins):
        a = ins[0][0]
        o = ins[0][0]
        for s, _c in ins[1:]:
            a = a & s
            o = o | s
        empty = a == 0
        return np.where(empty, o, a), sum(c for _s, c in ins) + empty

    def _transform(self, v):
        return np.min(v[None, :, :] + self.cost[:, :, None], axis=1)

    def _views(self, first, nbr, root):
        """up[v]: the subtree at v seen from its dad; down[v]: the rest of the tree seen from v"""
        n = self.n
        order, parent = rooted(first, nbr, n, root)
        zero = np.zeros(self.P, dtype=np.int64)
        fitch = self.cost is None
        leaf = (lambda t: (self.sets[t - 1], zero)) if fitch else (lambda t: self.tips[t - 1])
        up, down = {}, {}
        for dad, v in reversed(order):
            if v <= n:
                up[v] = leaf(v)
            else:
                kids = [up[u] for u in neighbours(first, nbr, n, v) if u != dad]
                up[v] = self._fitch(kids) if fitch else sum(self._transform(k) for k in kids)
        for dad, v in order:
            if dad == root:
                down[v] = leaf(root)
            if v <= n:
                continue
            lst = neighbours(first, nbr, n, v)
            ins = [down[v] if u == dad else up[u] for u in lst]
            d = len(ins)
            if fitch:
                # prefix / suffix accumulations of AND and OR: all inputs but the k-th is prefix[k] combined with suffix[k + 1]
                full = np.full(self.P, -1, dtype=np.int64)
                pa, po, sa, so = [full], [zero], [full] * (d + 1), [zero] * (d + 1)
                for s, _c in ins:
                    pa.append(pa[-1] & s)
                    po.append(po[-1] | s)
                for k in range(d - 1, -1, -1):
                    sa[k] = sa[k + 1] & ins[k][0]
                    so[k] = so[k + 1] | ins[k][0]
                steps = sum(c for _s, c in ins)
                for k, u in enumerate(lst):
                    if u == dad:
                        continue
                    a, o = pa[k] & sa[k + 1], po[k] | so[k + 1]
                    empty = a == 0
                    down[u] = (np.where(empty, o, a), steps - ins[k][1] + empty)
            else:
                tr = [self._transform(x) for x in ins]
                pre = [np.zeros_like(tr[0])]
                for x in tr:
                    pre.append(pre[-1] + x)
                suf = [np.zeros_like(tr[0])] * (d + 1)
                for k in range(d - 1, -1, -1):
                    suf[k] = suf[k + 1] + tr[k]
                for k, u in enumerate(lst):
                    if u != dad:
                        down[u] = pre[k] + suf[k + 1]
        return order, up, down

    def parsimony(self, first, nbr, root=1):
        """-> (length, _pattern_pars[P]) of computeParsimony() at the root leaf; 0 for a pattern not kept"""
        order, up, down = self._views(first, nbr, root)
        r0 = order[0][1]
        if self.cost is None:
            ptn = up[r0][1] + ((up[r0][0] & self.sets[root - 1]) == 0)
        else:
            ptn = np.min(up[r0] + self._transform(self.tips[root - 1]), axis=0)     # the rest of the tree is the parent side
        if self.keep is not None:
            ptn = ptn * self.keep
        return int((ptn * self.w).sum()), ptn

    def substitutions(self, first, nbr, root=1):
        """-> (branches, subst[int64]): computeParsimonyBranch's branch_subst of every branch, fixNegativeBranch's order"""
        order, up, down = self._views(first, nbr, root)
        out = []
        for dad, v in order:
            if self.cost is None:
                out.append(int((((up[v][0] & down[v][0]) == 0) * self.w).sum()))
            else:
                # dad_branch = the subtree at node2 enters as it is, node_branch = the rest transformed; a leaf node2 swaps the two
                par, kid = (down[v], up[v]) if v <= self.n else (up[v], down[v])
                out.append(int((np.min(par + self._transform(kid), axis=0) * self.w).sum()))
        return order, np.array(out, dtype=np.int64)


# ---------------------------------------------------------------- the second witness: per pattern, recursive, plain Python
def _rec_fitch(first, nbr, n, tipset, node, dad):
    """phylotree.cpp:869-931 for ONE pattern: (set, steps) of the subtree at node seen from dad"""
    if node <= n:
        return tipset[node - 1], 0                                 # external node: its states, subtree score 0
    partial = -1                                                    # memset(.., 255, ..)
    steps = 0
    kids = []
    for u in neighbours(first, nbr, n, node):                      # FOR_NEIGHBOR_IT(node, dad, it)
        if u == dad:
            continue
        child, child_steps = _rec_fitch(first, nbr, n, tipset, u, node)
        partial &= child                                            # partial_pars_dad[i] &= partial_pars_child[i]
        steps += child_steps
        kids.append(child)
    if partial == 0:                                                # isEmptyBitsEntry
        for child in kids:                                          # unionBitsEntry over every child
            partial |= child
        steps += 1                                                  # one step, whatever the degree
    return partial, steps


def _rec_snk(first, nbr, n, S, cost, tipcost, node, dad):
    """parstree.cpp:191-214 for ONE pattern: the cost row of the subtree at node seen from dad"""
    if node <= n:
        return tipcost[node - 1]
    partial = [0] * S
    for u in neighbours(first, nbr, n, node):
        if u == dad:
            continue
        child = _rec_snk(first, nbr, n, S, cost, tipcost, u, node)
        for i in range(S):
            best = child[0] + cost[i][0]
            for j in range(1, S):
                best = min(best, child[j] + cost[i][j])
            partial[i] += best
    return partial


def _tip_neighbour(first, nbr, n, tip):
    return next(n + 1 + i for i in range(len(first) - 1) if tip in neighbours(first, nbr, n, n + 1 + i))


def recursive_fitch(codes, weights, datatype, first, nbr, root=1):
    """-> (length, pattern_pars list, branches, subst list) with every side of every branch from its own recursion"""
    n, P = codes.shape
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 200))
    sets = tip_sets(codes, datatype)
    order, _parent = rooted(first, nbr, n, root)
    r0 = _tip_neighbour(first, nbr, n, root)
    ptn, subst = [], [0] * len(order)
    for p in range(P):
        tipset = [int(sets[t][p]) for t in range(n)]
        s, c = _rec_fitch(first, nbr, n, tipset, r0, root)
        ptn.append(c + (1 if (s & tipset[root - 1]) == 0 else 0))
        for b, (v1, v2) in enumerate(order):
            s2, _ = _rec_fitch(first, nbr, n, tipset, v2, v1)
            s1, _ = _rec_fitch(first, nbr, n, tipset, v1, v2)
            if (s1 & s2) == 0:
                subst[b] += int(weights[p])
    return sum(int(weights[p]) * ptn[p] for p in range(P)), ptn, order, subst


def recursive_weighted(codes, weights, datatype, cost, first, nbr, root=1):
    n, P = codes.shape
    S = 20 if datatype == 1 else 4
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 200))
    sets = tip_sets(codes, datatype)
    c = [[int(x) for x in row] for row in closed(cost)]
    big = max(max(row) for row in c) + 1
    order, _parent = rooted(first, nbr, n, root)
    r0 = _tip_neighbour(first, nbr, n, root)

    def across(par, kid):                                           # min_i( par[i] + min_j( kid[j] + cost[i][j] ) )
        return min(par[i] + min(kid[j] + c[i][j] for j in range(S)) for i in range(S))

    ptn, subst = [], [0] * len(order)
    for p in range(P):
        tipcost = [[0 if (int(sets[t][p]) >> k) & 1 else big for k in range(S)] for t in range(n)]
        ptn.append(across(_rec_snk(first, nbr, n, S, c, tipcost, r0, root), tipcost[root - 1]))
        for b, (v1, v2) in enumerate(order):
            sub = _rec_snk(first, nbr, n, S, c, tipcost, v2, v1)
            rest = _rec_snk(first, nbr, n, S, c, tipcost, v1, v2)
            subst[b] += int(weights[p]) * (across(rest, sub) if v2 <= n else across(sub, rest))
    return sum(int(weights[p]) * ptn[p] for p in range(P)), ptn, order, subst


# ---------------------------------------------------------------- shared inputs of the CPU and GPU tests
def star(n):
    """one inner node joined to every tip, tips in order"""
    return np.array([0, n], dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)


def random_collapse(back, n, rng, fraction):
    """(first, nbr) of the binary tree with about `fraction` of its inner branches contracted"""
    from mpboot_amd import trees
    inner = [(v, int(back[3 * v + s]) // 3) for v in range(n + 1, 2 * n - 1) for s in range(3) if int(back[3 * v + s]) // 3 > v]
    pick = [br for br in inner if rng.random() < fraction]
    return trees.collapse_branches(back, n, pick)


# malformed trees for the validator: (name, n, first, nbr); GOOD5 is a caterpillar of five taxa (inner nodes 6, 7, 8)
GOOD5 = ([0, 3, 6, 9], [1, 2, 7, 3, 6, 8, 7, 4, 5])
MALFORMED = [
    ("degree two", 5, [0, 2, 6], [1, 7, 6, 2, 3, 4]),
    ("asymmetric", 5, [0, 3, 6, 9], [1, 2, 7, 3, 6, 8, 6, 4, 5]),
    ("tip twice", 5, [0, 3, 6, 9], [1, 1, 7, 3, 6, 8, 7, 4, 5]),
    ("tip missing", 5, [0, 3, 6, 9], [1, 2, 7, 3, 6, 8, 7, 4, 4]),
    ("neighbour twice", 5, [0, 3, 6], [1, 7, 7, 6, 6, 2]),
    ("cycle: one edge too many", 6, [0, 4, 7, 12], [1, 2, 8, 9, 3, 7, 9, 4, 5, 6, 7, 8]),
    ("triangle and a node apart", 6, [0, 3, 6, 9, 12], [8, 9, 1, 7, 9, 2, 7, 8, 3, 4, 5, 6]),
    ("out of range", 5, [0, 3, 6, 9], [1, 2, 9, 3, 6, 8, 7, 4, 5]),
    ("own neighbour", 5, [0, 3, 6, 9], [1, 2, 6, 3, 6, 8, 7, 4, 5]),
    ("too many inner nodes", 5, [0, 3, 6, 9, 12], [1, 2, 7, 3, 6, 8, 7, 4, 9, 8, 5, 5]),
    ("first[0]", 5, [1, 3, 6, 9], [1, 2, 7, 3, 6, 8, 7, 4, 5]),
    ("no inner node", 5, [0], []),
]
