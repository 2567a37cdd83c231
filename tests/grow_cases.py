"""Inputs for k_grow (csrc/grow.hip) whose tree is DESIGNED, and plain references for them.  No device is needed here.

The addition kernel always starts from the three-taxon tree, so the data alone decide which trees it walks.  perfect_alignment
writes two-state columns, one or more per split of a designed unrooted tree: such columns are pairwise compatible, so
  * the length of the tree after every step is the number of columns that show both states among the taxa added so far
    (closed_form_lengths) -- whatever the ties do, because a tree that displays the columns' splits always has a branch where the
    next taxon costs nothing beyond the columns it makes variable;
  * with EVERY inner split supported each taxon has exactly one such branch: no ties, no draws, and the tree after every step is
    the induced subtree of the design (design_splits == tree_splits at the end);
  * splits left unsupported make ties (the lcg64 stream is drawn from), taxa that no supported split separates are identical: a
    cluster whose subtree costs nothing, which stepwiseAddition's descent cut does not enter.
plan_figures restates steps (1)-(3) of the kernel's plan for a tree: S, the skeleton, the number of parts, the deepest level at
which a node with both children walked sits (the level its second child's U is parked at: kGrowParkSkel), the longest root path.

A designed tree is a nested pair of labels below the start tip, which is label 0; arrange() hands the labels to alignment rows
so that, for the addition order of a seed, label 0 is the tip the reference starts from (the smallest of the first three taxa)."""
from __future__ import annotations

import functools
import types

import numpy as np

DNA, AA, GENERIC = 0, 1, 3          # mpf datatypes (engine.DNA, engine.AA, engine.GENERIC)
PARK_SKEL, MAX_PARTS, PARK_PART = 512, 1024, 64      # kGrowParkSkel, kGrowMaxParts, kGrowParkPart (grow.hpp)


# ---- the addition order of a seed: makePermutationFast with PLL's randum() (restated from oracle/rng.h; the host file pins it
# against Oracle.make_tree(seed, 0))
def _randum(seed):
    s0, s1, s2 = seed & 4095, (seed >> 12) & 4095, (seed >> 24) & 255
    t = 1549 * s0
    n0 = t & 4095
    t = (t >> 12) + 1549 * s1 + 406 * s0
    n1 = t & 4095
    t = (t >> 12) + 1549 * s2 + 406 * s1
    n2 = t & 255
    return (n2 << 24) | (n1 << 12) | n0, 0.00390625 * (n2 + 0.000244140625 * (n1 + 0.000244140625 * n0))


def addition_order(n, seed):
    """taxon numbers (1-based) in the order the addition loop takes them"""
    perm = list(range(n + 2))
    for i in range(1, n + 1):
        seed, d = _randum(seed)
        k = int((n + 1 - i) * d)
        perm[i], perm[i + k] = perm[i + k], perm[i]
    return perm[1:n + 1]


def arrange(n, seed, order=None, last=(), shuffle_seed=1):
    """labels in addition order -> (perm, start tip number, label of every row).  `order` lists all labels with 0 among the first
    three; left out, the labels are shuffled with 0 first and `last` at the end.  Label 0 goes to the smallest of the first three
    taxa: the tip the tree is hung from."""
    perm = addition_order(n, seed)
    if order is None:
        rest = [x for x in range(1, n) if x not in set(last)]
        np.random.default_rng(shuffle_seed).shuffle(rest)
        order = [0] + rest + list(last)
    order = list(order)
    assert sorted(order) == list(range(n)) and 0 in order[:3]
    i0, j = order.index(0), int(np.argmin(perm[:3]))
    order[i0], order[j] = order[j], order[i0]
    label_of_row = np.empty(n, dtype=np.int64)
    for i in range(n):
        label_of_row[perm[i] - 1] = order[i]
    return perm, min(perm[:3]), label_of_row


# ---- designed trees
def _cat(labels):
    t = (labels[-2], labels[-1]) if len(labels) > 1 else labels[0]
    for x in reversed(labels[:-2]):
        t = (x, t)
    return t


def _spine(items):
    t = (items[-2], items[-1])
    for x in reversed(items[:-2]):
        t = (x, t)
    return t


def caterpillar(n):
    """labels in spine order: 0 is the start tip, n - 2 and n - 1 the cherry at the far end"""
    return _cat(list(range(1, n)))


def caterpillar_with_forks(spine, fork_tips):
    """`spine` single tips, then a node -- at depth `spine` below the start tip's neighbour -- with a caterpillar of fork_tips[0] and
    one of fork_tips[1] tips as children.  Returns (tree, n); the last label is a tip of the second fork child."""
    a, b = fork_tips
    la = list(range(spine + 1, spine + 1 + a))
    lb = list(range(spine + 1 + a, spine + 1 + a + b))
    return _spine(list(range(1, spine + 1)) + [_cat(la), _cat(lb)]), 1 + spine + a + b


def cherry_caterpillar(n):
    """a spine of cherries (a single tip closes an odd count): the shape that leaves most parts, one per cherry"""
    lab = list(range(1, n))
    items = [(lab[i], lab[i + 1]) for i in range(0, len(lab) - 1, 2)]
    if len(lab) % 2:
        items.append(lab[-1])
    return _spine(items)


def caterpillar_with_clusters(sizes):
    """spine items from the start tip on: 1 = a tip, k > 1 = a cluster of k taxa (a caterpillar; unsupport its inner splits and
    the k taxa are identical).  Returns (tree, n, clusters as label lists, depth of every item's parent node)."""
    items, clusters, nxt = [], [], 1
    for k in sizes:
        lab = list(range(nxt, nxt + k))
        nxt += k
        items.append(_cat(lab))
        if k > 1:
            clusters.append(lab)
    depth = [min(i, len(sizes) - 2) for i in range(len(sizes))]
    return _spine(items), nxt, clusters, depth


def random_design(n, seed):
    """a tree of no particular shape (n small): the labels below the start tip split at random, recursively"""
    rng = np.random.default_rng(seed)

    def build(lab):
        if len(lab) == 1:
            return lab[0]
        k = int(rng.integers(1, len(lab)))
        return (build(lab[:k]), build(lab[k:]))
    return build(list(range(1, n)))


def design_splits(tree, n):
    """the n - 3 inner splits of the design as bool rows over the labels: the side without label 0, in post-order"""
    rows, vals, stack = [], [], [(tree, False)]
    while stack:
        node, done = stack.pop()
        if not isinstance(node, tuple):
            v = np.zeros(n, dtype=bool)
            v[node] = True
            vals.append(v)
        elif not done:
            stack.append((node, True))
            stack.append((node[1], False))
            stack.append((node[0], False))
        else:
            b, a = vals.pop(), vals.pop()
            vals.append(a | b)
            rows.append(vals[-1])
    rows.pop()                                   # the start tip's own branch
    out = np.array(rows)
    assert out.shape == (n - 3, n) and (out.sum(1) >= 2).all() and (out.sum(1) <= n - 2).all() and not out[:, 0].any()
    return out


def inside(splits, labels):
    """indices of the splits that lie strictly inside a cluster"""
    m = np.zeros(splits.shape[1], dtype=bool)
    m[list(labels)] = True
    return [i for i in range(len(splits)) if not (splits[i] & ~m).any() and splits[i].sum() < m.sum()]


# ---- the alignment
def perfect_alignment(splits, n, per_split=1, unsupported=(), nsites=None, named=None, place=None, datatype=DNA):
    """codes [n, P] in label order.  Every supported split gets per_split two-state columns; with nsites the supported splits are
    gone through again until the alignment has that many columns.  named: {name: bool column over the labels} -- columns of the
    caller's own (at least two taxa on either side), put at the site positions place[name]; every other column fills the free
    positions in order.  The two states of column j rotate through all ordered pairs of the alphabet, so every state row is in use."""
    named = dict(named or {})
    place = dict(place or {})
    off = set(unsupported)
    keep = [i for i in range(len(splits)) if i not in off]
    cols = [splits[i] for i in keep for _ in range(per_split)]
    if nsites is not None:
        assert len(cols) + len(named) <= nsites
        k = 0
        while len(cols) + len(named) < nsites:
            cols.append(splits[keep[k % len(keep)]])
            k += 1
    P = len(cols) + len(named)
    col = [None] * P
    for name, v in named.items():
        v = np.asarray(v, dtype=bool)
        assert 2 <= v.sum() <= n - 2 and col[place[name]] is None
        col[place[name]] = v
    free = iter(cols)
    for j in range(P):
        if col[j] is None:
            col[j] = next(free)
    member = np.array(col).T                                  # [n, P]
    ns = {DNA: 4, AA: 20, GENERIC: 32}[datatype]
    pairs = np.array([(a, b) for a in range(ns) for b in range(ns) if a != b])
    ab = pairs[(np.arange(P) * 7) % len(pairs)]
    st = np.where(member, ab[:, 1][None, :], ab[:, 0][None, :]).astype(np.uint8)
    return (np.uint8(1) << st).astype(np.uint8) if datatype == DNA else st


def closed_form_lengths(codes, perm):
    """best[k] = length of the tree of the first k taxa of perm (k = 3 .. n; below 3 zero): the columns that show both states"""
    o = codes[np.asarray(perm) - 1]
    diff = o != o[0:1]
    var = diff.any(axis=0)
    first = diff.argmax(axis=0)[var]                          # position (0-based) of the taxon that makes the column variable
    n = len(perm)
    cum = np.cumsum(np.bincount(first, minlength=n))
    best = np.zeros(n + 1, dtype=np.int64)
    best[3:] = cum[2:]
    return best


def packing(nsites):
    """(live words, row pitch Wp) of the engine's packing for that many informative sites of weight one"""
    ce = (nsites + 31) // 32
    return ce, max(32, (ce + 31) // 32 * 32)


def grow_shape(grow_tile, datatype=DNA):
    """(words per tile, waves per workgroup) of k_grow's launch shape: quad tiles of 16 x VW words, word-major (0) 64 words;
    16 waves where a vector tile is at most two registers"""
    if datatype != DNA:
        return 16, 8
    return {0: (64, 8), 1: (16, 16), 2: (32, 16), 4: (64, 8), 8: (128, 8)}[grow_tile]


def tiles_of(Wp, grow_tile, datatype=DNA):
    w = grow_shape(grow_tile, datatype)[0]
    return (Wp + w - 1) // w


# ---- trees as the engine and the oracle hand them out: back[record], record = 3 * node + k, tips 1 .. n
def _nx(r):
    return 3 * (r // 3) + (r % 3 + 1) % 3


class Rooted:
    """the tree hung from the start tip as k_grow holds it: pre-order (children in the reference's visiting order), subtree sizes"""

    def __init__(self, back, n, start_tip):
        back = np.asarray(back)
        rec, par = [], []
        stack = [(int(back[3 * start_tip]), -1)]
        while stack:
            c, p = stack.pop()
            i = len(rec)
            rec.append(c)
            par.append(p)
            if c // 3 > n:
                stack.append((int(back[_nx(_nx(c))]), i))
                stack.append((int(back[_nx(c)]), i))
        self.n, self.start_tip = n, start_tip
        self.rec, self.par = np.array(rec), np.array(par)
        m = len(rec)
        assert m == 2 * n - 3
        self.tip = np.where(self.rec // 3 <= n, self.rec // 3, 0)        # tip number, 0 = inner
        size = np.ones(m, dtype=np.int64)
        for i in range(m - 1, 0, -1):
            size[par[i]] += size[i]
        self.size = size
        self.c1 = np.full(m, -1)
        self.c2 = np.full(m, -1)
        inner = np.nonzero(self.tip == 0)[0]
        self.c1[inner] = inner + 1
        self.c2[inner] = inner + 1 + size[inner + 1]

    def counts(self, mask):
        """tips of `mask` (bool over tip numbers 0 .. n) below every node"""
        cs = np.concatenate([[0], np.cumsum(np.where(self.tip > 0, mask[self.tip], False))])
        i = np.arange(len(self.rec))
        return cs[i + self.size] - cs[i]


def plan_figures(tree, start_tip, nw, tips=None):
    """steps (1)-(3) of a k_grow step on `tree` (a Rooted, or back / n in a tuple) cut down to the taxa `tips` (numbers, the start
    tip among them; None = all): what the kernel plans when the next taxon is to be added to that tree."""
    R = tree if isinstance(tree, Rooted) else Rooted(tree[0], tree[1], start_tip)
    n = R.n
    mask = np.zeros(n + 1, dtype=bool)
    mask[list(range(1, n + 1)) if tips is None else list(tips)] = True
    assert mask[start_tip]
    k = int(mask.sum())
    cnt = R.counts(mask)
    inner = R.tip == 0
    c1, c2 = np.where(inner, R.c1, 0), np.where(inner, R.c2, 0)
    present = np.where(inner, (cnt[c1] > 0) & (cnt[c2] > 0), cnt > 0)
    size = 2 * cnt - 1                                        # of the cut-down tree's node that stands for this one
    idx = np.arange(len(R.rec))
    before = np.cumsum(present) - present                     # present nodes in front of i in pre-order ...
    ended = np.cumsum(np.bincount((idx + R.size)[present], minlength=len(idx) + 1))[idx]      # ... whose subtree ends in front of i
    depth = before - ended                                    # present proper ancestors
    m = 2 * k - 3
    assert present.sum() == m
    S = min(max(m // (3 * nw), 8), PARK_PART)
    skel = present & (size > S)
    s1, s2 = size[c1], size[c2]
    if m > 1 and m <= S:
        nparts = 1
    else:
        nparts = int((skel & inner & (s1 > 1) & (s1 <= S)).sum() + (skel & inner & (s2 > 1) & (s2 <= S)).sum())
    both = skel & inner & (s1 > S) & (s2 > S)
    return types.SimpleNamespace(m=m, S=S, skeleton=R.rec[skel].tolist(), nskel=int(skel.sum()), nparts=nparts,
                                 max_lev=int(depth[both].max()) if both.any() else -1,
                                 max_path=int(depth[present].max()) + 1, depth=depth, present=present, rooted=R)


def walked_figures(back, n, start_tip, nw, perm, stride=1):
    """the largest figures over the trees the kernel walks while it builds `back` in the order perm: the trees of the first
    3 .. n - 1 taxa (every stride-th, and the last 64 all)"""
    R = Rooted(back, n, start_tip)
    ks = sorted(set(range(3, n, stride)) | set(range(max(3, n - 64), n)))
    out = types.SimpleNamespace(max_lev=-1, nparts=0, max_path=0, nskel=0)
    for k in ks:
        f = plan_figures(R, start_tip, nw, perm[:k])
        out.max_lev, out.nparts = max(out.max_lev, f.max_lev), max(out.nparts, f.nparts)
        out.max_path, out.nskel = max(out.max_path, f.max_path), max(out.nskel, f.nskel)
    return out


def tree_splits(back, n, start_tip):
    """the inner splits of a tree as a set: the side without the start tip, as packed bits over the rows"""
    R = Rooted(back, n, start_tip)
    out = set()
    below = np.zeros((len(R.rec), n), dtype=bool)
    for i in range(len(R.rec) - 1, 0, -1):
        if R.tip[i]:
            below[i, R.tip[i] - 1] = True
        else:
            out.add(np.packbits(below[i]).tobytes())
        below[R.par[i]] |= below[i]
    return out


def clade(R, tips):
    """(the tips form a clade, depth of its root below the start tip's neighbour, pre-order index of the root)"""
    mask = np.zeros(R.n + 1, dtype=bool)
    mask[list(tips)] = True
    cnt = R.counts(mask)
    i = int(np.nonzero(cnt == len(tips))[0].max())            # the deepest node above all of them
    allm = np.ones(R.n + 1, dtype=bool)
    depth, j = 0, R.par[i]
    while j >= 0:
        depth, j = depth + 1, R.par[j]
    return int(R.counts(allm)[i]) == len(tips), depth, i


# ---- the cases of tests/test_gpu_grow_edges.py; tests/test_grow_cases_host.py proves each one's figure from the oracle's tree
def _case(name, tree, n, seed, datatype=DNA, tie_seed=3, order=None, last=(), **aln):
    splits = design_splits(tree, n)
    perm, start_tip, label_of_row = arrange(n, seed, order=order, last=last)
    by_label = perfect_alignment(splits, n, datatype=datatype, **aln)
    off = sorted(set(aln.get("unsupported", ())))
    sup = np.array([i for i in range(len(splits)) if i not in set(off)], dtype=np.int64)
    return types.SimpleNamespace(name=name, n=n, seed=seed, tie_seed=tie_seed, datatype=datatype, perm=perm, start_tip=start_tip,
                                 label_of_row=label_of_row, row_of_label=np.argsort(label_of_row),
                                 codes=np.ascontiguousarray(by_label[label_of_row]), nsites=by_label.shape[1],
                                 supported=splits[sup][:, label_of_row], all_supported=not off and not aln.get("named"),
                                 closed=None, open_splits=0)


def _finish(c):
    c.closed = closed_form_lengths(c.codes, c.perm)
    c.design = {np.packbits(r).tobytes() for r in c.supported}
    return c


FORK_TIPS = (35, 35)         # a fork child keeps 34 tips = 67 nodes > S in the last tree the kernel walks


@functools.lru_cache(maxsize=None)
def depth_case(fork_depth):
    """A: a caterpillar with a fork at the far end, every split supported.  The fork node sits at depth fork_depth and both its
    children are walked by the skeleton: its second child's U is parked at level fork_depth.  The last taxon added is a fork
    tip, so the fork is at its full depth in the last tree the kernel walks."""
    tree, n = caterpillar_with_forks(fork_depth, FORK_TIPS)
    c = _finish(_case(f"fork at depth {fork_depth}", tree, n, seed=11, last=(n - 1,)))
    c.fork_depth = fork_depth
    return c


@functools.lru_cache(maxsize=None)
def size_case(n):
    """B: a caterpillar of cherries, every split supported (n - 3 columns)"""
    return _finish(_case(f"cherry caterpillar {n}", cherry_caterpillar(n) if n > 5 else caterpillar(n), n, seed=5))


CUT_SIZES = [1] * 185
for _i, _k in {20: 3, 68: 3, 72: 4, 76: 5, 100: 6, 140: 4, 146: 3, 152: 4, 165: 5}.items():
    CUT_SIZES[_i] = _k
CUT_OPEN = sorted(set(range(5, 125, 3)) | {40, 41, 42, 70, 71, 72, 140})      # spine items whose branch towards the start tip has no column
CUT_SITES = {"plain": 149 * 32 + 29, "first word": 150 * 32, "last word of the last tile": 150 * 32, "last partial word": 149 * 32 + 1}


@functools.lru_cache(maxsize=None)
def cut_case(variant):
    """C: a caterpillar of 214 taxa with nine clusters of 3-6 identical taxa at design depths 20 .. 165 (in the oracle's trees:
    either side of 64 and of 128), 45 spine branches without a column.  Wp = 160, 150 live words: two tiles at least for every
    DNA shape, the last live word in every shape's last tile.  Variants: two taxa of the five-taxon cluster next to depth 64
    differ from the other three by ONE column -- in the first word, in the last live word, or as the only site of the last
    partial word -- and one of them is the first of the cluster to be added: the subtree costs something from its second taxon
    on, and the other of the two has its one best branch inside it."""
    tree, n, clusters, depth = caterpillar_with_clusters(CUT_SIZES)
    splits = design_splits(tree, n)
    off = [i for cl in clusters for i in inside(splits, cl)]
    first_label = np.concatenate([[0], np.cumsum(CUT_SIZES)[:-1]]) + 1            # of every spine item
    for it in CUT_OPEN:                                       # the split "this item and everything behind it"
        want = np.zeros(n, dtype=bool)
        want[first_label[it]:] = True
        off.append(int(np.nonzero((splits == want).all(axis=1))[0][0]))
    nsites = CUT_SITES[variant]
    named, place, order = None, None, None
    dev = clusters[3]                                         # the cluster of five taxa next to depth 64
    if variant != "plain":
        v = np.zeros(n, dtype=bool)
        v[[dev[1], dev[2]]] = True
        named = {"dev": v}
        place = {"dev": {"first word": 3, "last word of the last tile": nsites - 5, "last partial word": nsites - 1}[variant]}
        rest = [x for x in range(1, n)]
        np.random.default_rng(2).shuffle(rest)
        at = sorted(rest.index(x) for x in dev)               # the cluster's places in the order: dev[1] first, dev[2] third
        for p, x in zip(at, [dev[1], dev[0], dev[2], dev[3], dev[4]]):
            rest[p] = x
        order = [0] + rest
    c = _finish(_case(f"cut: {variant}", tree, n, seed=21, tie_seed=5, order=order, unsupported=off, nsites=nsites, named=named, place=place))
    if named:
        c.supported = np.concatenate([c.supported, named["dev"][None, c.label_of_row]])
        c.design = {np.packbits(r).tobytes() for r in c.supported}
    c.clusters = [[int(c.row_of_label[x]) + 1 for x in cl] for cl in clusters]       # as tip numbers
    c.cluster_depth = [depth[i] for i, k in enumerate(CUT_SIZES) if k > 1]
    c.open_splits = len(CUT_OPEN)
    c.costly = 3 if variant != "plain" else None              # index of the cluster whose subtree costs something
    return c


@functools.lru_cache(maxsize=None)
def early_cluster_case(n):
    """C, the flags' running count: the start tree costs something, the fourth and the fifth taxon are identical to the second.
    After the first insertion exactly one inner node has a subtree without a mutation -- the new one, which is the first entry of
    its own root path."""
    tree, n_, clusters, _ = caterpillar_with_clusters([3] + [1] * (n - 4))
    assert n_ == n
    splits = design_splits(tree, n)
    c = _finish(_case(f"early cluster {n}", tree, n, seed=9, tie_seed=2, order=[0, 1, 4, 2, 3] + list(range(5, n)),
                      unsupported=inside(splits, clusters[0]), per_split=3))
    c.clusters = [[int(c.row_of_label[x]) + 1 for x in clusters[0]]]
    return c


TAIL_WP = {32: 31, 64: 63, 96: 95, 160: 159}                  # row pitch -> full words in front of the last one: every word of the row is live


@functools.lru_cache(maxsize=None)
def tail_case(Wp, rem, datatype=DNA):
    """D: 24 taxa, a tree of no particular shape, four splits without a column.  Three more splits (a cherry, a clade of five and
    one of eleven where the design has them) have their columns ONLY in the last live word, which holds rem sites (0 = all 32):
    the taxa those splits place are decided there alone.  The last live word is the last word of the row: the word that lanes
    past the row end are clamped to."""
    n = 24
    tree = random_design(n, 4)
    splits = design_splits(tree, n)
    sz = splits.sum(axis=1)
    by_size = np.argsort(np.abs(sz - 11), kind="stable")
    tail = [int(np.nonzero(sz == 2)[0][0]), int(np.argsort(np.abs(sz - 5), kind="stable")[0]), int(by_size[0])]
    assert len(set(tail)) == 3
    off = [i for i in range(len(splits)) if i not in tail][2:18:4]
    live = rem if rem else 32
    nsites = TAIL_WP[Wp] * 32 + live
    named = {f"tail{j}": splits[tail[j % 3]] for j in range(live)}
    place = {f"tail{j}": TAIL_WP[Wp] * 32 + j for j in range(live)}
    lost = tail[live:]                                        # (one site: one of the three splits only)
    c = _finish(_case(f"tail Wp {Wp} rem {rem} type {datatype}", tree, n, seed=17, tie_seed=4, datatype=datatype,
                      unsupported=off + tail, nsites=nsites, named=named, place=place))
    c.supported = np.concatenate([c.supported, splits[[t for t in tail if t not in lost]][:, c.label_of_row]])
    c.design = {np.packbits(r).tobytes() for r in c.supported}
    c.Wp, c.open_splits = Wp, len(off)
    return c


@functools.lru_cache(maxsize=None)
def noisy_case(datatype=DNA):
    """D with homoplasy: the same 24-taxon design, 48 columns that fit no tree (a random half of the taxa each) among the split
    columns.  With compatible columns alone an up-vector taken from the wrong child washes out one level further down; here it
    does not.  The closed form does not hold: the references are the host's loop and the oracle."""
    n = 24
    tree = random_design(n, 4)
    splits = design_splits(tree, n)
    rng = np.random.default_rng(6)
    named, place = {}, {}
    for j in range(48):
        v = np.zeros(n, dtype=bool)
        v[rng.choice(n, size=int(rng.integers(4, n - 3)), replace=False)] = True
        named[f"noise{j}"], place[f"noise{j}"] = v, 21 * j + 5
    c = _case(f"homoplasy type {datatype}", tree, n, seed=17, tie_seed=4, datatype=datatype, unsupported=[3, 9], nsites=31 * 32 + 17,
              named=named, place=place)
    c.closed = closed_form_lengths(c.codes, c.perm)            # (a lower bound here)
    c.noisy = True
    return c


# ---- what the two test files go through
DEPTHS = (PARK_SKEL - 1, PARK_SKEL)
CUT_VARIANTS = tuple(CUT_SITES)
DNA_TILES = (0, 1, 2, 4, 8)
CUT_TILES = {0: 3, 1: 10, 2: 5, 4: 3, 8: 2}                   # workgroups at Wp = 160
TAIL_DNA = [(t, Wp, {(0, 32): 1, (0, 96): 2, (1, 32): 2, (1, 96): 6, (2, 32): 1, (2, 96): 3, (4, 32): 1, (4, 96): 2,
                     (8, 32): 1, (8, 96): 1, (8, 160): 2}[(t, Wp)])
            for t in DNA_TILES for Wp in ((32, 96, 160) if t == 8 else (32, 96))]       # (grow_tile, Wp, workgroups)
TAIL_OTHER = [(dt, Wp, Wp // 16) for dt in (AA, GENERIC) for Wp in (32, 64)]
REMS = (0, 1, 31)                                             # sites in the last live word (0: all 32)


def all_cases():
    out = [depth_case(d) for d in DEPTHS] + [size_case(n) for n in (4, 5, 2048, 2049)] + [cut_case(v) for v in CUT_VARIANTS]
    out += [early_cluster_case(8)]
    out += [tail_case(Wp, r) for Wp in (32, 96, 160) for r in REMS] + [tail_case(Wp, r, dt) for dt, Wp, _ in TAIL_OTHER for r in REMS]
    return out


_ORACLE = {}


def oracle_reference(c, tie_seed=None):
    """the oracle's stepwise addition of a case, computed once: per-step lengths, insertion branches, tree, score, tie state"""
    key = (c.name, tie_seed)
    if key not in _ORACLE:
        from oracle import pyoracle as po
        o = po.Oracle(c.codes, datatype=c.datatype)
        o.seed_ties(po.TIE_RANDOM, c.tie_seed if tie_seed is None else tie_seed)
        seeded = o.tie_state()
        score, best, ins = o.stepwise(c.seed)
        _ORACLE[key] = dict(score=score, best=best.tolist(), ins=ins.tolist(), tree=o.get_tree().tolist(), tie_state=o.tie_state(),
                            seeded=seeded, sites=o.num_informative, rows=o.S)
    return _ORACLE[key]
