"""Python restatement of the split products on trees with polytomies, for the tests of the mpf_*_set calls and of the host-only
program: a tree is either a record array (trees.splits) or a (first, nbr) pair of neighbour lists (splits_witness.list_splits), its
splits are Python frozensets, RF is the size of the symmetric difference.  Written independently of
mpboot_amd/host/split_sets.hpp: never words, never DFS intervals."""
from collections import Counter

import numpy as np

import splits_witness as sw
from mpboot_amd import trees


def is_lists(t):
    return isinstance(t, tuple)


def inner_branches(back, n):
    """the n - 3 inner branches of a binary tree as (node, node), smaller node first"""
    out = []
    for v in range(n + 1, 2 * n - 1):
        for s in range(3):
            u = int(back[3 * v + s]) // 3
            if u > v:
                out.append((v, u))
    return out


def collapse(back, n, k, rng):
    """`back` with k of its inner branches (drawn without replacement) contracted -> (first, nbr)"""
    br = inner_branches(back, n)
    pick = rng.choice(len(br), size=k, replace=False) if k else []
    return trees.collapse_branches(back, n, [br[int(i)] for i in pick])


def star(n):
    return np.array([0, n], dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)


def middle_hub(n):
    """tip 1 and tip 2 on one inner node, every other tip on a second one: a node of degree n - 1 in the middle, one split"""
    return np.array([0, 3, n + 2], dtype=np.int32), np.array([1, 2, n + 2, n + 1] + list(range(3, n + 1)), dtype=np.int32)


def splits_of(t, n):
    """the non-trivial splits of a tree of either form, as a frozenset of frozensets (the side without tip 1)"""
    if not is_lists(t):
        return frozenset(trees.splits(np.asarray(t)))
    below = sw.list_splits(t[0], t[1], n)
    return frozenset(s for s in below.values() if len(s) < n - 1)


def split_sets(items, n):
    return [splits_of(t, n) for t in items]


def all_pairs(sets):
    out = np.zeros((len(sets), len(sets)), dtype=np.int32)
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            out[i, j] = out[j, i] = len(sets[i] ^ sets[j])
    return out


def adjacent(sets):
    return np.array([len(sets[i] ^ sets[i + 1]) for i in range(len(sets) - 1)], dtype=np.int32)


def two_sets(a, b):
    return np.array([[len(x ^ y) for y in b] for x in a], dtype=np.int32).reshape(len(a), len(b))


def counts(sets, weights=None):
    c, total = Counter(), 0
    for i, s in enumerate(sets):
        w = 1 if weights is None else int(weights[i])
        if w == 0:
            continue
        total += w
        for x in s:
            c[x] += w
    return c, total


def ordered_table(sets, weights, n):
    """([words tuple], [count], total) in the contract order"""
    c, total = counts(sets, weights)
    o = sw.contract_order(c, n)
    return [sw.set_words(s, n) for s, _ in o], [k for _, k in o], total


def consensus(sets, weights, threshold, n):
    c, total = counts(sets, weights)
    return sw.build_lists(sw.greedy(sw.contract_order(c, n), total, threshold, n), n), total


def branch_walk(first, nbr, n):
    """[(node1, node2)] in the order of polytomy_branch_substitutions from tip 1: pre-order, neighbours in list order"""
    first = [int(x) for x in first]
    nbr = [int(x) for x in nbr]
    adj = {n + 1 + i: nbr[first[i]:first[i + 1]] for i in range(len(first) - 1)}
    root = next(v for v, a in adj.items() if 1 in a)
    out, stack = [], [(root, 1)]
    while stack:
        v, dad = stack.pop()
        out.append((dad, v))
        if v > n:
            stack.extend((u, v) for u in reversed(adj[v]) if u != dad)
    return out


def supports(sets, weights, target, n):
    """[(node1, node2, support)] of the list tree `target` in branch_walk order: -1 on a leaf branch and on the branch at tip 1"""
    c, _ = counts(sets, weights)
    below = sw.list_splits(target[0], target[1], n)
    out = []
    for a, b in branch_walk(target[0], target[1], n):
        out.append((a, b, -1 if b <= n or a == 1 else c.get(below[b], 0)))
    return out


def mixed_family(n, N, seed, max_moves=3):
    """N related trees on n taxa (splits_witness.related_trees); a random half of them contracted by 1 .. n - 3 branches, tree 1 the star,
    tree 0 kept in record format -> list of items (record array | (first, nbr))"""
    backs = sw.related_trees(n, N, seed, max_moves)
    rng = np.random.default_rng(seed + 1000)
    items = []
    for i, b in enumerate(backs):
        if i == 0 or n < 4:
            items.append(b)
        elif i == 1:
            items.append(star(n))
        elif rng.integers(0, 2):
            items.append(collapse(b, n, int(rng.integers(1, n - 2)), rng))
        else:
            items.append(b)
    return items


def as_engine_args(items):
    """(backs, lists, permutation): the engine takes the records first, then the lists; permutation[k] = the item at set index k"""
    rec = [i for i, t in enumerate(items) if not is_lists(t)]
    lst = [i for i, t in enumerate(items) if is_lists(t)]
    return [items[i] for i in rec] or None, [items[i] for i in lst] or None, rec + lst


def write_sets(path, n, mode, items, items2=(), weights=None):
    """the program's input file; weights in the order of `items` (the file wants them in set order: records, then lists)"""
    def one(f, its):
        rec = [t for t in its if not is_lists(t)]
        lst = [t for t in its if is_lists(t)]
        if rec:
            np.asarray(rec, dtype=np.int32).tofile(f)
        np.array([len(t[0]) - 1 for t in lst], dtype=np.int32).tofile(f)
        for k in (0, 1):
            for t in lst:
                np.asarray(t[k], dtype=np.int32).tofile(f)

    def n_of(its):
        return [sum(1 for t in its if not is_lists(t)), sum(1 for t in its if is_lists(t))]

    with open(path, "wb") as f:
        np.array([n, mode, int(weights is not None)] + n_of(items) + n_of(items2), dtype=np.int32).tofile(f)
        one(f, items)
        one(f, items2)
        if weights is not None:
            perm = as_engine_args(list(items))[2]
            np.array([weights[i] for i in perm], dtype=np.int32).tofile(f)
    return path


BROKEN = ("degree_two", "asymmetric", "missing_tip", "tip_twice", "cycle", "two_components")


def broken_lists(kind):
    """one defect each in the lists of ((1,2),3,4,(5,6),(7,8,9)) on 9 taxa -- inner nodes 10 (the hub), 11, 12, 13; "good": none"""
    adj = {10: [11, 3, 4, 12, 13], 11: [10, 1, 2], 12: [10, 5, 6], 13: [10, 7, 8, 9]}
    if kind == "degree_two":
        adj[12], adj[13] = [10, 5, 6, 8, 9], [10, 7]
    elif kind == "asymmetric":
        adj[12] = [11, 5, 6]                          # 10 lists 12, 12 lists 11 instead
    elif kind == "missing_tip":
        adj[13] = [10, 7, 8]
    elif kind == "tip_twice":
        adj[12] = [10, 5, 6, 9]
    elif kind == "cycle":
        # 11 - 12 - 13 - 11 closed and cut off from the rest: as many edges as a tree has, every tip once
        adj = {10: [3, 4, 14], 11: [12, 1, 13], 12: [11, 5, 13], 13: [12, 7, 11], 14: [10, 2, 6, 8, 9]}
    elif kind == "two_components":
        adj = {10: [1, 2, 3, 4], 11: [5, 6, 7, 8, 9]}
    else:
        assert kind == "good"
    first, nbr = [0], []
    for v in sorted(adj):
        nbr += adj[v]
        first.append(len(nbr))
    return np.array(first, dtype=np.int32), np.array(nbr, dtype=np.int32)
