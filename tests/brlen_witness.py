"""Witness of mpboot's parsimony branch lengths -- TEST INFRASTRUCTURE ONLY.

A plain restatement of PhyloTree::fixNegativeBranch (reference phylotree.cpp:3597-3633) over the record links back[] the engine uses
(record = 3 * node + slot, node number = IQ-TREE id + 1, slot = position in neighbors[]):

  * the walk: pre-order from the root leaf, neighbours other than dad in slot order, each branch met once from its root side;
    node1 = the end nearer the root, node2 the other end;
  * Fitch (PhyloTree::computeParsimonyBranch, phylotree.cpp:938-1047): branch_subst = sum over patterns of frequency x [the state
    sets of the two sides have no state in common].  The sets of both sides of every branch come from two passes written here: one
    post-order pass for the sides away from the root, one pre-order pass for the sides towards it; the count is formed pattern by
    pattern.  Nothing is taken from the engine or from oracle/;
  * ParsTree (parstree.cpp:439-541): branch_subst = tree_pars, the weighted length of the tree rooted at the branch -- the
    edge-rooted DP of tests/nni_snk_witness.py (SnkScorer), dad_branch = the subtree at node2 entering as it is, node_branch = the
    rest of the tree transformed; a leaf node2 swaps the two (:449-457);
  * the length from the count (phylotree.cpp:3608-3614) in numpy double precision.
"""
import numpy as np

MIN_BRANCH_LEN = 1e-6                                 # phylotree.h:35


def fitch_tip_sets(codes, datatype):
    """PLL tip codes -> state sets as bit masks (datatype: 0 DNA, 1 protein, 2 binary, 3 multistate)"""
    c = np.asarray(codes, dtype=np.int64)
    if datatype in (0, 2):
        return c
    if datatype == 3:
        return np.where(c < 32, np.left_shift(1, np.minimum(c, 31)), (1 << 32) - 1)
    m = np.where(c < 20, np.left_shift(1, np.minimum(c, 19)), (1 << 20) - 1)
    m = np.where(c == 20, (1 << 2) | (1 << 3), m)
    return np.where(c == 21, (1 << 5) | (1 << 6), m)


def deg(n, v):
    return 3 if v > n else 1


def branch_order(back, n, root_taxon=1):
    """[(node1, node2)] in fixNegativeBranch's order, 2 n - 3 entries"""
    out, st = [], [(root_taxon, 0)]
    while st:
        node, dad = st.pop()
        if dad:
            out.append((dad, node))
        for s in reversed(range(deg(n, node))):
            w = int(back[3 * node + s]) // 3
            if w != dad:
                st.append((w, node))
    return out


def _rec(back, n, a, b):
    """the record at node a whose neighbour is node b"""
    return next(3 * a + s for s in range(deg(n, a)) if int(back[3 * a + s]) // 3 == b)


def _join(x, y):
    sx, cx = x
    sy, cy = y
    inter = sx & sy
    empty = inter == 0
    return np.where(empty, sx | sy, inter), cx + cy + empty


def fitch_sides(codes, datatype, back, n, root_taxon=1):
    """for every branch in order: ((set, steps) of the side at node2, (set, steps) of the side at node1), per pattern"""
    sets = fitch_tip_sets(codes, datatype)
    P = sets.shape[1]
    order = branch_order(back, n, root_taxon)
    zero = np.zeros(P, dtype=np.int64)
    children = {}                                     # node -> its neighbours away from the root, slot order
    for v1, v2 in order:
        children.setdefault(v1, []).append(v2)
    down = {}                                         # node -> (set, steps) of the subtree at node, seen from its dad
    for v1, v2 in reversed(order):                    # post-order: a node's children come behind it in the pre-order
        if v2 <= n:
            down[v2] = (sets[v2 - 1], zero)
        else:
            a, b = children[v2]
            down[v2] = _join(down[a], down[b])
    up = {}                                           # node -> (set, steps) of the rest of the tree, seen from node
    for v1, v2 in order:                              # pre-order
        if v1 == root_taxon:
            up[v2] = (sets[v1 - 1], zero)
        else:
            sib = next(c for c in children[v1] if c != v2)
            up[v2] = _join(up[v1], down[sib])
    return order, [(down[v2], up[v2]) for _v1, v2 in order]


def fitch_substitutions(codes, weights, datatype, back, n, root_taxon=1, keep=None):
    """-> (order, subst[int64], total[int64]): subst[i] = the branch's weighted count over the kept patterns, formed pattern by
    pattern; total[i] = steps(side 1) + steps(side 2) + subst[i], the tree length as that branch sees it"""
    w = np.asarray(weights, dtype=np.int64)
    if keep is not None:
        w = w * (np.asarray(keep) != 0)
    order, sides = fitch_sides(codes, datatype, back, n, root_taxon)
    subst, total = [], []
    for (s2, c2), (s1, c1) in sides:
        k = tot = 0
        for p in range(len(w)):
            e = 1 if (int(s1[p]) & int(s2[p])) == 0 else 0
            k += int(w[p]) * e
            tot += int(w[p]) * (int(c1[p]) + int(c2[p]) + e)
        subst.append(k)
        total.append(tot)
    return order, np.array(subst, dtype=np.int64), np.array(total, dtype=np.int64)


def fitch_substitutions_fast(codes, weights, datatype, back, n, root_taxon=1, keep=None):
    """the same counts with the per-pattern sum left to numpy (the size pins)"""
    w = np.asarray(weights, dtype=np.int64)
    if keep is not None:
        w = w * (np.asarray(keep) != 0)
    order, sides = fitch_sides(codes, datatype, back, n, root_taxon)
    return order, np.array([int((((s1 & s2) == 0) * w).sum()) for (s2, _c2), (s1, _c1) in sides], dtype=np.int64)


def weighted_values(scorer, back, n, root_taxon=1, reverse=False):
    """-> (order, value[int64]) with an SnkScorer: the tree rooted at each branch in ParsTree::computeParsimonyBranch's orientation
    (reverse: the other one)"""
    order = branch_order(back, n, root_taxon)
    out = []
    for v1, v2 in order:
        swap = (v2 <= n) != reverse                   # a leaf node2: the leaf is the transformed side
        out.append(scorer.edge_length(back, v2, v1) if swap else scorer.edge_length(back, v1, v2))
    return order, np.array(out, dtype=np.int64)


def lengths(subst, n_sites, n_states):
    """phylotree.cpp:3608-3614 in double precision"""
    s = np.asarray(subst, dtype=np.float64)
    N = np.float64(n_sites)
    bl = np.where(s > 0, s / N, np.float64(1.0) / N)
    z = np.float64(n_states) / np.float64(n_states - 1)
    x = np.float64(1.0) - z * bl
    with np.errstate(invalid="ignore", divide="ignore"):
        bl = np.where(x > 0, -np.log(np.where(x > 0, x, 1.0)) / z, bl)
    return np.maximum(bl, MIN_BRANCH_LEN)
