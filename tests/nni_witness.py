"""Witness of mpboot's NNI hill climb in MP mode -- TEST INFRASTRUCTURE ONLY.

A plain restatement of IQTree::optimizeNNI (reference iqtree.cpp:2173-2302) with the MP defaults (Fitch, nni5 off,
leastSquareNNI off), over the record links back[] the engine uses: record = 3 * node + slot, node number = IQ-TREE id + 1,
slot = position in neighbors[].  Every NNI is scored by doing the swap, scoring the whole tree with a scorer given by the
caller (the pinned oracle's score_tree) and swapping back -- nothing is taken from the engine.

  * getBestNNIForBran (phylotree.cpp:3807-3980): a = node1's first neighbour other than node2 in slot order, b the other,
    c0 / c1 node2's two others in slot order; move k swaps a with c_k; move 0 if len0 < len1, else move 1.
  * evalNNIs() (iqtree.cpp:3144-3159): pre-order from the root tip, neighbours in slot order, branch (node, dad).
  * speednni (updateBrans2Eval, :2304-2311, getInBranches mtree.cpp:816-827): std::map<string, Branch>, key = lower id and
    higher id written one behind the other, first insert wins, evaluated in key order.
  * plusNNIs sorted by libstdc++ std::sort (introsort, threshold 16, median of three, final insertion sort) with
    len_a < len_b (NNIMove::operator<, phylotree.h:225); genNonconfNNIs (:3020-3035) greedy.
"""
import numpy as np


# ---------------------------------------------------------------- libstdc++ std::sort (bits/stl_algo.h, bits/stl_heap.h)
def _lg(n):
    return n.bit_length() - 1


def _adjust_heap(a, first, hole, length, value, less):
    top = hole
    second = hole
    while second < (length - 1) // 2:
        second = 2 * (second + 1)
        if less(a[first + second], a[first + second - 1]):
            second -= 1
        a[first + hole] = a[first + second]
        hole = second
    if (length & 1) == 0 and second == (length - 2) // 2:
        second = 2 * (second + 1)
        a[first + hole] = a[first + second - 1]
        hole = second - 1
    parent = (hole - 1) // 2
    while hole > top and less(a[first + parent], value):
        a[first + hole] = a[first + parent]
        hole = parent
        parent = (hole - 1) // 2
    a[first + hole] = value


def _heap_sort(a, first, last, less):
    length = last - first
    if length >= 2:                                   # make_heap
        parent = (length - 2) // 2
        while True:
            _adjust_heap(a, first, parent, length, a[first + parent], less)
            if parent == 0:
                break
            parent -= 1
    while last - first > 1:                           # sort_heap
        last -= 1
        value = a[last]
        a[last] = a[first]
        _adjust_heap(a, first, 0, last - first, value, less)


def _move_median_to_first(a, result, x, y, z, less):
    if less(a[x], a[y]):
        if less(a[y], a[z]):
            m = y
        elif less(a[x], a[z]):
            m = z
        else:
            m = x
    elif less(a[x], a[z]):
        m = x
    elif less(a[y], a[z]):
        m = z
    else:
        m = y
    a[result], a[m] = a[m], a[result]


def _unguarded_partition(a, first, last, pivot, less):
    while True:
        while less(a[first], a[pivot]):
            first += 1
        last -= 1
        while less(a[pivot], a[last]):
            last -= 1
        if not first < last:
            return first
        a[first], a[last] = a[last], a[first]
        first += 1


def _introsort_loop(a, first, last, depth, less):
    while last - first > 16:
        if depth == 0:
            _heap_sort(a, first, last, less)          # partial_sort(first, last, last)
            return
        depth -= 1
        mid = first + (last - first) // 2
        _move_median_to_first(a, first, first + 1, mid, last - 1, less)
        cut = _unguarded_partition(a, first + 1, last, first, less)
        _introsort_loop(a, cut, last, depth, less)
        last = cut


def _unguarded_linear_insert(a, i, less):
    val = a[i]
    j = i - 1
    while less(val, a[j]):
        a[i] = a[j]
        i = j
        j -= 1
    a[i] = val


def _insertion_sort(a, first, last, less):
    for i in range(first + 1, last):
        if less(a[i], a[first]):
            val = a[i]
            a[first + 1:i + 1] = a[first:i]
            a[first] = val
        else:
            _unguarded_linear_insert(a, i, less)


def std_sort(a, less):
    """std::sort(a.begin(), a.end(), less) of libstdc++, in place on a Python list"""
    n = len(a)
    if n < 2:
        return a
    _introsort_loop(a, 0, n, 2 * _lg(n), less)
    if n > 16:
        _insertion_sort(a, 0, 16, less)
        for i in range(16, n):
            _unguarded_linear_insert(a, i, less)
    else:
        _insertion_sort(a, 0, n, less)
    return a


# ---------------------------------------------------------------- the climb
class NniWitness:
    def __init__(self, back, n, score_fn, root_taxon=1):
        self.back = np.array(back, dtype=np.int32).copy()
        self.n = n
        self.score_fn = score_fn                      # back[] -> Fitch length
        self.root = root_taxon
        self.log = []                                 # (node1, slot1, node2, slot2) of every swap, reverts included
        self.rollbacks = 0

    def nb(self, v, s):
        return int(self.back[3 * v + s]) // 3

    def deg(self, v):
        return 3 if v > self.n else 1

    def swap(self, mv, log=True):
        v1, s1, v2, s2 = mv
        p, q = 3 * v1 + s1, 3 * v2 + s2
        rp, rq = int(self.back[p]), int(self.back[q])
        self.back[p], self.back[rq] = rq, p
        self.back[q], self.back[rp] = rp, q
        if log:
            self.log.append(tuple(mv))

    def full_order(self):
        out, st = [], [(self.root, 0)]
        while st:
            node, dad = st.pop()
            if node > self.n and dad > self.n:
                out.append((node, dad))
            for s in reversed(range(self.deg(node))):
                w = self.nb(node, s)
                if w != dad:
                    st.append((w, node))
        return out

    def branch_moves(self, v1, v2):
        s1 = [s for s in range(3) if self.nb(v1, s) != v2]
        s2 = [s for s in range(3) if self.nb(v2, s) != v1]
        return [(v1, s1[0], v2, s2[0]), (v1, s1[0], v2, s2[1])]

    def score_branch(self, v1, v2):
        """(len0, len1, move0, move1): each move done, the tree scored, the move undone"""
        lens = []
        mvs = self.branch_moves(v1, v2)
        for mv in mvs:
            self.swap(mv, log=False)
            lens.append(int(self.score_fn(self.back)))
            self.swap(mv, log=False)
        return lens[0], lens[1], mvs[0], mvs[1]

    def scores(self):
        """one full evaluation: [(node1, node2, len0, len1)]"""
        out = []
        for v1, v2 in self.full_order():
            l0, l1, _, _ = self.score_branch(v1, v2)
            out.append((v1, v2, l0, l1))
        return out

    def _in_branches(self, brans, depth, node, dad):
        if depth == 0:
            return
        for s in range(3):
            w = self.nb(node, s)
            if w == dad or w <= self.n:
                continue
            self._add(brans, node, w)
            self._in_branches(brans, depth - 1, w, node)

    @staticmethod
    def _add(brans, x, y):
        lo, hi = min(x, y), max(x, y)
        key = (str(lo - 1) + str(hi - 1)).encode()
        if key not in brans:
            brans[key] = (lo, hi)

    def optimize(self, speednni=True, max_steps=50):
        """-> (length, nni_count, nni_steps)"""
        cur = int(self.score_fn(self.back))
        brans = {}
        rollback = False
        count = 0
        num = 0
        chosen = []
        step = 1
        while step <= max_steps:
            old = cur
            if not rollback:
                if speednni and brans:
                    order = [brans[k] for k in sorted(brans)]       # std::map<std::string>: byte order of the keys
                else:
                    order = self.full_order()
                plus = []
                for v1, v2 in order:
                    l0, l1, m0, m1 = self.score_branch(v1, v2)
                    ln, mv = (l0, m0) if l0 < l1 else (l1, m1)
                    if ln < cur:
                        plus.append((ln, mv))
                std_sort(plus, lambda a, b: a[0] < b[0])
                if not plus:
                    break
                chosen = []
                for ln, mv in plus:
                    if all(mv[0] != c[1][0] and mv[2] != c[1][0] and mv[0] != c[1][2] and mv[2] != c[1][2] for c in chosen):
                        chosen.append((ln, mv))
                num = len(chosen)
            for i in range(num):
                self.swap(chosen[i][1])
            if speednni:
                brans = {}
                for i in range(num):
                    v1, _, v2, _ = chosen[i][1]
                    self._add(brans, v1, v2)
                    self._in_branches(brans, 2, v1, v2)
                    self._in_branches(brans, 2, v2, v1)
            cur = int(self.score_fn(self.back))
            if cur <= chosen[0][0]:
                count += num
                rollback = False
            else:
                for i in range(num):
                    self.swap(chosen[i][1])
                rollback = True
                num = 1
                cur = old
                self.rollbacks += 1
            step += 1
        return cur, count, step
