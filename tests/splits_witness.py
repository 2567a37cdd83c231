"""Python restatement of the bootstrap summary, for the tests of mpf_split_counts / mpf_split_support / mpf_consensus_tree and of the
host-only program: the splits of a weighted tree set from trees.splits (frozensets, recursive), the contract order, the reference's
consensus rule (drop count <= threshold * total, then SplitGraph::findMaxCompatibleSplits) and the neighbour lists of the kept sets.
Written independently of mpboot_amd/host/split_sets.hpp: sets are Python frozensets here, never words."""
from collections import Counter

import numpy as np

from mpboot_amd import trees


def words_of(n):
    return (n + 31) // 32


def set_words(s, n):
    w = [0] * words_of(n)
    for t in s:
        w[(t - 1) >> 5] |= 1 << ((t - 1) & 31)
    return tuple(w)


def words_set(w):
    return frozenset(32 * j + b + 1 for j, x in enumerate(w) for b in range(32) if int(x) >> b & 1)


def counts(backs, weights=None):
    """(Counter {frozenset: summed weight}, total weight); a tree of weight 0 contributes nothing"""
    c, total = Counter(), 0
    for i, b in enumerate(backs):
        w = 1 if weights is None else int(weights[i])
        if w == 0:
            continue
        total += w
        for s in trees.splits(np.asarray(b)):
            c[s] += w
    return c, total


def contract_order(counter, n):
    """[(frozenset, count)] by count descending, then the words ascending as unsigned, word 0 first"""
    return sorted(counter.items(), key=lambda kv: (-kv[1], set_words(kv[0], n)))


def compatible(a, b):
    return not (a & b) or a <= b or b <= a


def greedy(ordered, total, threshold, n):
    """the kept [(frozenset, count)] of the consensus rule on a list in the contract order"""
    kept = []
    cut = float(threshold) * float(total)
    for s, c in ordered:
        if len(kept) >= n - 3:
            break
        if float(c) <= cut:
            continue
        if all(compatible(s, k) for k, _ in kept):
            kept.append((s, c))
    return kept


def build_lists(kept, n):
    """(first, nbr, support_of_inner) of the tree whose non-trivial splits are the kept sets: tips 1 .. n, inner nodes n + 1 .. in
    pre-order from tip 1, each inner node lists its parent, then its children by their smallest tip"""
    root = frozenset(range(2, n + 1))
    sets = [root] + [s for s, _ in kept]
    count = {s: c for s, c in kept}
    parent = {}
    for s in sets[1:]:
        parent[s] = min((p for p in sets if s < p), key=len)
    kids = {s: [] for s in sets}
    for s in sets[1:]:
        kids[parent[s]].append(s)
    first, nbr, sup = [0], [], []
    number, order, chs = {}, [], {}
    # numbers are given in pre-order (an explicit stack: a caterpillar is n deep); the lists are written once every node has one
    stack = [root]
    while stack:
        s = stack.pop()
        number[s] = n + 1 + len(order)
        order.append(s)
        own = set(s)
        for k in kids[s]:
            own -= k
        chs[s] = sorted([(min(k), k) for k in kids[s]] + [(t, t) for t in own], key=lambda x: x[0])
        stack.extend(k for _, k in reversed(chs[s]) if isinstance(k, frozenset))
    for s in order:
        nbr.append(1 if s == root else number[parent[s]])
        for _, k in chs[s]:
            nbr.append(number[k] if isinstance(k, frozenset) else k)
        first.append(len(nbr))
        sup.append(-1 if s == root else count[s])
    return first, nbr, sup


def list_splits(first, nbr, n):
    """{inner node: frozenset of the tips below it, seen from tip 1} of a tree given as neighbour lists; the node next to tip 1 included"""
    first = [int(x) for x in first]
    nbr = [int(x) for x in nbr]
    adj = {n + 1 + i: nbr[first[i]:first[i + 1]] for i in range(len(first) - 1)}
    root = next(v for v, a in adj.items() if 1 in a)
    below = {}
    stack = [(root, 1, False)]
    while stack:
        v, dad, done = stack.pop()
        if not done:
            stack.append((v, dad, True))
            stack.extend((u, v, False) for u in adj[v] if u != dad and u > n)
        else:
            s = set()
            for u in adj[v]:
                if u == dad:
                    continue
                s |= below[u] if u > n else {u}
            below[v] = frozenset(s)
    return below


def caterpillar(n):
    """the deepest walk from tip 1: (1, 2, (3, (4, (... (n - 1, n)))))"""
    names = [str(i) for i in range(1, n + 1)]
    s = str(n - 1) + "," + str(n)
    for t in range(n - 2, 2, -1):
        s = str(t) + ",(" + s + ")"
    return trees.newick_to_back("(1,2,(" + s + "));", names)


def balanced(n):
    """as balanced as n allows: halve the tip list recursively"""
    names = [str(i) for i in range(1, n + 1)]

    def sub(lst):
        if len(lst) == 1:
            return lst[0]
        h = len(lst) // 2
        return "(" + sub(lst[:h]) + "," + sub(lst[h:]) + ")"

    a = n // 3
    b = (n - a) // 2
    return trees.newick_to_back("(" + sub(names[:a]) + "," + sub(names[a:a + b]) + "," + sub(names[a + b:]) + ");", names)


def random_spr(back, n, rng):
    """one trees.apply_spr move drawn uniformly: prune record p of an inner node, regraft on a branch outside the pruned subtree that
    does not touch p's node"""
    b = np.asarray(back, dtype=np.int32)
    while True:
        v = int(rng.integers(n + 1, 2 * n - 1))
        p = 3 * v + int(rng.integers(0, 3))
        q = int(rng.integers(3, 3 * (2 * n - 1)))
        if b[q] < 0:
            continue
        inside, st = set(), [int(b[p])]
        while st:
            r = st.pop()
            inside.add(r // 3)
            if r // 3 > n:
                st += [int(b[trees.nxt(r)]), int(b[trees.nxt(trees.nxt(r))])]
        ends = (q // 3, int(b[q]) // 3)
        if v in ends or inside & set(ends):
            continue
        out = trees.apply_spr(b, p, q)
        trees.validate(out, n)
        return out


def related_trees(n, k, seed, max_moves=3):
    """k trees, each 0 .. max_moves random SPR moves away from one random tree"""
    rng = np.random.default_rng(seed)
    base = trees.random_topology(n, rng)
    out = []
    for _ in range(k):
        b = base.copy()
        for _ in range(int(rng.integers(0, max_moves + 1))):
            b = random_spr(b, n, rng)
        out.append(b)
    return out


def cyclic_records(back, n):
    """records that still link both ways everywhere but are no tree: two inner branches cut and joined crosswise so that one part
    closes into a cycle and the other falls off (what the back-link check of mpf_set_tree alone does not see)"""
    b = np.asarray(back, dtype=np.int32).copy()
    for v in range(n + 1, 2 * n - 1):
        for s0 in range(3):
            r1 = 3 * v + s0
            e = int(b[r1])                                  # the far end of the first branch
            if e // 3 <= n:
                continue
            for mid in (int(b[trees.nxt(e)]), int(b[trees.nxt(trees.nxt(e))])):
                if mid // 3 <= n:
                    continue
                for r2 in (int(b[trees.nxt(mid)]), int(b[trees.nxt(trees.nxt(mid))])):
                    if r2 // 3 <= n:
                        continue
                    x = int(b[r2])                          # second branch: r2 (far side) -- x (near side)
                    b[r1], b[r2] = r2, r1
                    b[e], b[x] = x, e
                    return b
    raise AssertionError("no two inner branches in a row")
