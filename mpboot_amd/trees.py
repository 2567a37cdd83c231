"""Flat unrooted-binary-tree topologies in the engine's record convention.

A topology over n taxa is an int32 array ``back`` of length ``3*(2n-1)``:
record ``rec = 3*v + s`` is slot ``s`` (0..2) of node ``v``; tips are nodes
1..n (slot 0 only), inner nodes n+1..2n-2 (three slots in cyclic order
s -> (s+1)%3, the analogue of PLL's ``next`` ring, pllrepo/src/pll.h:622-701);
``back[rec]`` is the record across the branch (PLL's ``back``), -1 if unused.
"""
from __future__ import annotations

import numpy as np


def n_taxa_of(back: np.ndarray) -> int:
    return (len(back) // 3 + 1) // 2


def empty_back(n: int) -> np.ndarray:
    return np.full(3 * (2 * n - 1), -1, dtype=np.int32)


def nxt(rec: int) -> int:
    v, s = divmod(rec, 3)
    return 3 * v + (s + 1) % 3


def validate(back: np.ndarray, n: int | None = None) -> None:
    n = n or n_taxa_of(back)
    assert len(back) == 3 * (2 * n - 1)
    for v in range(1, 2 * n - 1):
        for s in range(1 if v <= n else 3):
            r = 3 * v + s
            b = int(back[r])
            assert b >= 3 and back[b] == r, f"broken link at rec {r}"
    # connectivity
    seen = set()
    stack = [3]
    while stack:
        r = stack.pop()
        v = r // 3
        if v in seen:
            continue
        seen.add(v)
        for s in range(1 if v <= n else 3):
            stack.append(int(back[3 * v + s]))
    assert len(seen) == 2 * n - 2, "tree is not connected"


def parse_newick(s: str):
    """-> nested lists of leaf names (branch lengths / inner labels dropped)."""
    s = s.strip().rstrip(";")
    pos = 0

    def node():
        nonlocal pos
        if s[pos] == "(":
            pos += 1
            kids = [node()]
            while s[pos] == ",":
                pos += 1
                kids.append(node())
            assert s[pos] == ")"
            pos += 1
            skip_label()
            return kids
        start = pos
        while s[pos] not in ",():;" if pos < len(s) else False:
            pos += 1
        name = s[start:pos]
        skip_len()
        return name

    def skip_len():
        nonlocal pos
        if pos < len(s) and s[pos] == ":":
            pos += 1
            while pos < len(s) and s[pos] not in ",()":
                pos += 1

    def skip_label():
        nonlocal pos
        while pos < len(s) and s[pos] not in ",():":
            pos += 1
        skip_len()

    t = node()
    return t


def newick_to_back(nwk: str, names: list[str]) -> np.ndarray:
    n = len(names)
    tip = {nm: i + 1 for i, nm in enumerate(names)}
    t = parse_newick(nwk)
    if len(t) == 2:       # rooted: dissolve the root
        a, b = t
        if isinstance(a, list):
            t = a + [b]
        else:
            t = b + [a]
    assert len(t) == 3, "need a binary tree"
    back = empty_back(n)
    counter = [n + 1]

    def link(a, b):
        back[a] = b
        back[b] = a

    def build(sub, parent_rec):
        if isinstance(sub, str):
            link(3 * tip[sub], parent_rec)
            return
        assert len(sub) == 2, "need a binary tree"
        v = counter[0]
        counter[0] += 1
        link(3 * v, parent_rec)
        build(sub[0], 3 * v + 1)
        build(sub[1], 3 * v + 2)

    root = counter[0]
    counter[0] += 1
    for s, sub in enumerate(t):
        build(sub, 3 * root + s)
    validate(back, n)
    return back


def back_to_newick(back: np.ndarray, names: list[str], start_tip: int = 1) -> str:
    n = len(names)

    def sub(rec):           # subtree hanging behind record rec (looking away from back[rec])
        v = rec // 3
        if v <= n:
            return names[v - 1]
        a, b = nxt(rec), nxt(nxt(rec))
        return "(" + sub(int(back[a])) + "," + sub(int(back[b])) + ")"

    r = int(back[3 * start_tip])
    v = r // 3
    if v <= n:
        return f"({names[start_tip - 1]},{names[v - 1]});"
    a, b = nxt(r), nxt(nxt(r))
    return f"({names[start_tip - 1]},{sub(int(back[a]))},{sub(int(back[b]))});"


def random_topology(n: int, rng: np.random.Generator) -> np.ndarray:
    """Random stepwise addition (uniform branch each step)."""
    back = empty_back(n)
    order = rng.permutation(n) + 1
    v = n + 1
    a, b, c = (int(x) for x in order[:3])
    for s, t in enumerate((a, b, c)):
        back[3 * v + s] = 3 * t
        back[3 * t] = 3 * v + s
    edges = [3 * a, 3 * b, 3 * c]          # one record per edge
    for t in order[3:]:
        t = int(t)
        v += 1
        e = edges[int(rng.integers(len(edges)))]
        f = int(back[e])
        back[3 * v] = 3 * t
        back[3 * t] = 3 * v
        back[3 * v + 1] = e
        back[e] = 3 * v + 1
        back[3 * v + 2] = f
        back[f] = 3 * v + 2
        edges.append(3 * t)
        edges.append(3 * v + 2)
    validate(back, n)
    return back


def splits(back: np.ndarray) -> frozenset:
    """Non-trivial bipartitions as frozensets of tip ids on the side not containing tip 1."""
    n = n_taxa_of(back)
    out = set()

    def tips_behind(rec):
        v = rec // 3
        if v <= n:
            return frozenset([v])
        a, b = nxt(rec), nxt(nxt(rec))
        s = tips_behind(int(back[a])) | tips_behind(int(back[b]))
        if 1 < len(s) < n - 1:
            out.add(s if 1 not in s else frozenset(range(1, n + 1)) - s)
        return s

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * n + 100))
    try:
        tips_behind(int(back[3]))
    finally:
        sys.setrecursionlimit(old)
    return frozenset(out)


def parse_topology_line(tokens: list[str], n: int) -> np.ndarray:
    """'rec:back' tokens as printed by oracle/ref_driver.c -> back array."""
    back = empty_back(n)
    for tok in tokens:
        r, b = tok.split(":")
        back[int(r)] = int(b)
    return back


def apply_spr(back: np.ndarray, p: int, q: int) -> np.ndarray:
    """Prune node record p (it keeps the subtree behind back[p]) and regraft it on branch (q, back[q])
    -- removeNodeParsimony + insertParsimony of the reference (sprparsimony.cpp:2245-2257, :1942-1952)."""
    b = np.array(back, dtype=np.int32).copy()
    a1, a2 = int(b[nxt(p)]), int(b[nxt(nxt(p))])
    b[a1], b[a2] = a2, a1
    r = int(b[q])
    b[nxt(p)], b[q] = q, nxt(p)
    b[nxt(nxt(p))], b[r] = r, nxt(nxt(p))
    return b


def apply_tbr(back: np.ndarray, p: int, f: int, g: int) -> np.ndarray:
    """Cut the edge (p, q = back[p]) and join the middle of branch (f, back[f]) of q's part to the middle of branch (g, back[g])
    of p's part; -1 for either means that part's own root.  Two apply_spr steps on disjoint links (no reference function: MPBoot
    has SPR and NNI only)."""
    b = np.array(back, dtype=np.int32).copy()
    q = int(b[p])
    if g >= 0:
        b = apply_spr(b, p, g)
    if f >= 0:
        b = apply_spr(b, q, f)
    return b


def random_spr_moves(engine_obj, back: np.ndarray, rng: np.random.Generator, k: int, maxtrav: int = 6) -> np.ndarray:
    """k random SPR moves within the given radius (a stand-in for the search's perturbation step): the prune node
    and the regraft branch are drawn uniformly from what rearrangeParsimony would test."""
    n = n_taxa_of(back)
    b = np.array(back, dtype=np.int32).copy()
    done = 0
    while done < k:
        v = int(rng.integers(n + 1, 2 * n - 1))
        rec = 3 * v + int(rng.integers(0, 3))
        engine_obj.set_tree(b)
        q, _mp, n_p = engine_obj.spr_scan(rec, 1, maxtrav)
        if n_p == 0:
            continue
        b = apply_spr(b, rec, int(q[int(rng.integers(0, n_p))]))
        done += 1
    return b


# ---------------------------------------------------------------- multifurcating trees as neighbour lists
def collapse_branches(back: np.ndarray, n: int, inner_branches=()):
    """Contract the given inner branches [(node, node), ...] of the binary tree `back` -> (first, nbr), the CSR neighbour lists
    the engine's polytomy calls take: tips stay nodes 1 .. n, the surviving inner nodes are renumbered n + 1 .. n + n_inner in
    the order of the smallest binary node number of each merged group, inner node i has the neighbours nbr[first[i]:first[i + 1]].
    Neighbour order is kept: a merged node lists what its smallest member lists, slot order, with every contracted neighbour
    replaced in place by that neighbour's other neighbours in its slot order behind the branch contracted (cyclically)."""
    pairs = {frozenset((int(a), int(b))) for a, b in inner_branches}
    for pr in pairs:
        assert len(pr) == 2 and all(n < v <= 2 * n - 2 for v in pr), "inner branches only"
    rep = list(range(2 * n - 1))

    def find(v):
        while rep[v] != v:
            rep[v] = rep[rep[v]]
            v = rep[v]
        return v

    for pr in pairs:
        a, b = sorted(find(v) for v in pr)
        assert any(int(back[3 * min(pr) + s]) // 3 == max(pr) for s in range(3)), "not a branch of the tree"
        rep[b] = a

    def others(v, frm):
        if frm is None:
            slots = (0, 1, 2)
        else:
            k = next(s for s in range(3) if int(back[3 * v + s]) // 3 == frm)
            slots = ((k + 1) % 3, (k + 2) % 3)
        return [(v, int(back[3 * v + s]) // 3) for s in slots]

    reps = sorted({find(v) for v in range(n + 1, 2 * n - 1)})
    number = {r: n + 1 + i for i, r in enumerate(reps)}
    first, nbr = [0], []
    for r in reps:
        stack = list(reversed(others(r, None)))
        while stack:
            v, u = stack.pop()
            if u > n and frozenset((v, u)) in pairs:
                stack.extend(reversed(others(u, v)))
            else:
                nbr.append(u if u <= n else number[find(u)])
        first.append(len(nbr))
    return np.array(first, dtype=np.int32), np.array(nbr, dtype=np.int32)


def lists_to_back(first, nbr, n: int) -> np.ndarray:
    """the record links of a tree whose inner nodes all have three neighbours (slot = position in the list)"""
    first = np.asarray(first)
    assert len(first) - 1 == n - 2 and (np.diff(first) == 3).all(), "a fully resolved tree only"
    back = empty_back(n)
    pos = {}
    for i in range(n - 2):
        for s in range(3):
            pos[(n + 1 + i, int(nbr[first[i] + s]))] = 3 * (n + 1 + i) + s
    for (v, u), r in pos.items():
        if u <= n:
            back[r] = 3 * u
            back[3 * u] = r
        else:
            back[r] = pos[(u, v)]
    return back


def back_to_lists(back, n: int):
    """(first, nbr) of the binary tree `back`: inner node n + 1 + i lists the nodes behind its three records in slot order -- the
    inverse of lists_to_back"""
    back = np.asarray(back)
    nbr = np.array([int(back[3 * v + s]) // 3 for v in range(n + 1, 2 * n - 1) for s in range(3)], dtype=np.int32)
    return np.arange(0, 3 * (n - 2) + 1, 3, dtype=np.int32), nbr


def insert_tip(first, nbr, n: int, tip: int, node1: int, node2: int):
    """(first, nbr) with `tip` attached in the middle of branch (node1, node2) the way PhyloTree::computeParsimonyTree rewires
    neighbors[] (phylotree.cpp:1243-1320): the new inner node -- number n + 1 + old n_inner, its list appended -- takes node1's
    place in node2's list and node2's place in node1's list, in place, and lists [tip, node2, node1] (node2 = target_node, the end
    away from the root leaf; node1 = target_dad)."""
    first = [int(x) for x in first]
    nbr = [int(x) for x in nbr]
    v = n + len(first)
    for at, what in ((node2, node1), (node1, node2)):
        if at > n:
            i = at - n - 1
            k = nbr.index(what, first[i], first[i + 1])
            nbr[k] = v
    nbr += [int(tip), int(node2), int(node1)]
    first.append(len(nbr))
    return np.array(first, dtype=np.int32), np.array(nbr, dtype=np.int32)


def drop_tips(tree, n: int, tips):
    """(first, nbr) of `tree` -- a record tree (back array) or a (first, nbr) pair -- with the leaves `tips` removed and every node
    left with two neighbours suppressed: the backbone of a reinsertion (FitchEngine.place_taxa).  Surviving inner nodes keep their
    relative order and are renumbered n + 1 ..; a neighbour that went away is replaced in place by what lay behind it."""
    if isinstance(tree, (tuple, list)):
        first, nbr = tree
    else:
        first, nbr = back_to_lists(tree, n)
    first = [int(x) for x in first]
    adj = {n + 1 + i: [int(u) for u in nbr[first[i]:first[i + 1]]] for i in range(len(first) - 1)}
    for t in tips:
        t = int(t)
        v = next(v for v, l in adj.items() if t in l)
        adj[v].remove(t)
        if len(adj[v]) == 2:                    # (its two neighbours keep their degree: nothing else to suppress)
            a, b = adj.pop(v)
            for x, y in ((a, b), (b, a)):
                if x > n:
                    adj[x][adj[x].index(v)] = y
    keep = sorted(adj)
    assert len(keep) >= 1 and all(len(adj[v]) >= 3 for v in keep), "fewer than three tips left"
    number = {v: n + 1 + i for i, v in enumerate(keep)}
    out_first, out_nbr = [0], []
    for v in keep:
        out_nbr += [u if u <= n else number[u] for u in adj[v]]
        out_first.append(len(out_nbr))
    return np.array(out_first, dtype=np.int32), np.array(out_nbr, dtype=np.int32)


def lists_to_newick(first, nbr, names: list[str], support=None) -> str:
    """Newick string of a tree given as neighbour lists (tips 1 .. n, inner node i = node n + 1 + i), written from tip 1 with the
    neighbours in list order.  support[i] (optional, per inner node): written as the label of inner node i where it is >= 0 --
    the form the consensus tree of the engine (consensus_tree: its split supports) goes to a .contree file in."""
    n = len(names)
    first = [int(x) for x in first]
    nbr = [int(x) for x in nbr]
    tip_nb = {}
    for i in range(len(first) - 1):
        for u in nbr[first[i]:first[i + 1]]:
            if u <= n:
                tip_nb[u] = n + 1 + i
    # iterative post-order from the inner node next to tip 1
    text = {}
    root = tip_nb[1]
    stack = [(root, 1, False)]
    while stack:
        v, dad, done = stack.pop()
        if v <= n:
            text[v] = names[v - 1]
            continue
        i = v - n - 1
        kids = [u for u in nbr[first[i]:first[i + 1]] if u != dad]
        if not done:
            stack.append((v, dad, True))
            stack.extend((u, v, False) for u in reversed(kids))
            continue
        label = "" if support is None or int(support[i]) < 0 else str(int(support[i]))
        if v == root:
            text[v] = "(" + ",".join([names[0]] + [text.pop(u) for u in kids]) + ")" + label + ";"
        else:
            text[v] = "(" + ",".join(text.pop(u) for u in kids) + ")" + label
    return text[root]
