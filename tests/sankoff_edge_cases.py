"""Inputs of the weighted (Sankoff) engine's edge-case tests: small deterministic constructors, no device, no engine.

tests/test_gpu_sankoff_edges.py runs them on the kernels, tests/test_oracle_sankoff.py checks on the CPU that the oracle's Sankoff
mode and the plain int64 reference (oracle/sankoff_slow.py) agree on the very same arrays.  A case is a dict:
  name, group, datatype, codes [n][P] uint8, weights [P] int32, cost [S][S] uint32 (the caller's matrix on the data type's own
  states), sym (the closed matrix is symmetric), back (start topology), ninf (informative columns by construction, or None),
  radii (scan radii), nodes (how many spread prune nodes are scanned; 0 = every one).
"""
import functools
import itertools

import numpy as np

from helpers import load_fixture
from mpboot_amd import trees
from oracle import sankoff_slow

DNA, AA, BIN, GENERIC = 0, 1, 2, 3
STATES = {DNA: 4, AA: 20, BIN: 2, GENERIC: 32}
UNDETERMINED = {DNA: 15, AA: 22, BIN: 3, GENERIC: 32}          # globalVariables.h pLengths
HEAVY = (100000, 65535, 0, 7, 1)                               # the weights every group A alignment carries


# ---- cost matrices
def unit_cost(S, scale=1):
    return ((1 - np.eye(S, dtype=np.int64)) * scale).astype(np.uint32)


def random_metric(S, seed):
    """L1 distances of random points: a metric, so the triangle closure leaves it as it is"""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, 12, size=(S, 3))
    c = np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2).astype(np.uint32)
    c[c == 0] = 1
    np.fill_diagonal(c, 0)
    return c


def random_asymmetric(S, seed):
    """step-matrix style costs: i -> j and j -> i differ; the closure leaves it asymmetric"""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 7, size=(S, S)).astype(np.uint32)
    c[np.triu_indices(S, 1)] += 2
    np.fill_diagonal(c, 0)
    return c


def metric_with_largest(S, largest, seed):
    """symmetric, every off-diagonal entry in [ceil(largest / 2), largest] and one of them == largest: any two entries sum to at
    least the third, so the matrix is its own closure"""
    rng = np.random.default_rng(seed)
    c = rng.integers((largest + 1) // 2, largest + 1, size=(S, S)).astype(np.uint32)
    c = np.minimum(c, c.T)
    c[0, S - 1] = c[S - 1, 0] = largest
    np.fill_diagonal(c, 0)
    return c


def closed_kernel_matrix(cost, datatype):
    """the matrix as the kernels carry it (Engine::create): binary data sits in the 4-row kernels, the rows no tip can have filled with
    largest + 1 BEFORE the closure; DNA, protein and multistate under a cost matrix keep their own 4 / 20 / 32 rows"""
    c = np.array(cost, dtype=np.int64)
    if datatype == BIN:
        k = np.full((4, 4), int(c.max()) + 1, dtype=np.int64)
        np.fill_diagonal(k, 0)
        k[:2, :2] = c
        c = k
    return sankoff_slow.close_triangle(c)


def expect_packed(cost, datatype, n):
    """the documented rule of the 16-bit store: 3 n highest_cost < 2^16, highest_cost = largest closed entry + 1"""
    highest = int(closed_kernel_matrix(cost, datatype).max()) + 1
    return 3 * n * highest < 65536, highest


def kernel_states(datatype):
    return {DNA: 4, BIN: 4, AA: 20, GENERIC: 32}[datatype]


# ---- alignments
def _single(datatype, k):
    return (1 << k) if datatype in (DNA, BIN) else k


def _ambiguous(datatype, rng):
    if datatype == DNA:
        return int(rng.choice([3, 5, 6, 7, 9, 10, 11, 12, 13, 14]))
    if datatype == AA:
        return int(rng.choice([20, 21]))
    return UNDETERMINED[datatype]


def edge_alignment(n, ninf, datatype, seed, all_different=0):
    """exactly `ninf` informative columns (two or more different determined codes), interleaved with columns the packing drops --
    constant ones, ones with a single determined taxon, all-undetermined ones -- so that the kept patterns' indices are not 0, 1, 2...
    The first `all_different` informative columns give the taxa states that differ as far as the alphabet allows.
    -> codes, weights, indices of the informative columns.  Weights: HEAVY on the first kept pattern, the last one, its pair partner
    in the 16-bit store (index ^ 1) and their neighbours; 1 .. 3 elsewhere, the dropped columns included."""
    rng = np.random.default_rng(seed)
    S, und = STATES[datatype], UNDETERMINED[datatype]
    cols, kept = [], []

    def filler(kind):
        c = np.full(n, und, dtype=np.uint8)
        if kind == 0:
            c[:] = _single(datatype, int(rng.integers(S)))
            c[int(rng.integers(n))] = und
        elif kind == 1:
            c[int(rng.integers(n))] = _single(datatype, int(rng.integers(S)))
        return c

    kinds = itertools.cycle((0, 1, 2))
    cols.append(filler(next(kinds)))
    for j in range(ninf):
        if j < all_different:
            c = np.array([_single(datatype, int(x) % S) for x in rng.permutation(n) + j], dtype=np.uint8)
        else:
            base = int(rng.integers(S))
            c = np.array([_single(datatype, base if rng.random() < 0.45 else int(rng.integers(S))) for _ in range(n)], dtype=np.uint8)
            if rng.random() < 0.3:
                c[int(rng.integers(n))] = _ambiguous(datatype, rng)
            if rng.random() < 0.2:
                c[int(rng.integers(n))] = und
            det = c[c < und]
            if len(set(det.tolist())) < 2:                     # keep it informative
                c[0], c[1] = _single(datatype, 0), _single(datatype, 1)
        kept.append(len(cols))
        cols.append(c)
        if j % 3 == 1 or j == ninf - 1:
            cols.append(filler(next(kinds)))
    codes = np.ascontiguousarray(np.stack(cols, axis=1))
    w = rng.integers(1, 4, size=codes.shape[1]).astype(np.int32)
    if ninf:
        last = ninf - 1
        spots = [p for p in dict.fromkeys([0, last, last ^ 1, 1, last - 2, last - 1]) if 0 <= p < ninf]
        for p, h in zip(spots, HEAVY[ninf % 5:] + HEAVY[:ninf % 5]):
            w[kept[p]] = h
    return codes, w, np.array(kept, dtype=np.int64)


# ---- topologies
def caterpillar(n):
    """((((t1,t2),t3),t4) ..., t_{n-1}, t_n): the deepest tree on n taxa"""
    names = [f"t{i + 1}" for i in range(n)]
    inner = "(t1,t2)"
    for i in range(3, n - 1):
        inner = f"({inner},t{i})"
    return trees.newick_to_back(f"({inner},t{n - 1},t{n});", names)


def balanced(n):
    """three perfectly balanced clades where n allows (64 = 16 + 16 + 32 taxa: depth 5 everywhere)"""
    names = [f"t{i + 1}" for i in range(n)]

    def sub(lo, hi):
        if hi - lo == 1:
            return names[lo]
        mid = (lo + hi) // 2
        return f"({sub(lo, mid)},{sub(mid, hi)})"

    q = n // 4
    return trees.newick_to_back(f"({sub(0, q)},{sub(q, 2 * q)},{sub(2 * q, n)});", names)


def all_topologies(n):
    """every unrooted binary topology on n taxa (3 * 5 * ... * (2n - 5) of them), taxa added in order to every branch"""
    out = []
    for choice in itertools.product(*[range(2 * k - 3) for k in range(3, n)]):
        back = trees.empty_back(n)
        v = n + 1
        for s, t in enumerate((1, 2, 3)):
            back[3 * v + s] = 3 * t
            back[3 * t] = 3 * v + s
        edges = [3, 6, 9]
        for t, pick in zip(range(4, n + 1), choice):
            v += 1
            e = edges[pick]
            f = int(back[e])
            back[3 * v], back[3 * t] = 3 * t, 3 * v
            back[3 * v + 1], back[e] = e, 3 * v + 1
            back[3 * v + 2], back[f] = f, 3 * v + 2
            edges += [3 * t, 3 * v + 2]
        trees.validate(back, n)
        out.append(back)
    return out


# ---- the cases
def _case(name, group, datatype, codes, weights, cost, back, ninf=None, radii=(3,), nodes=0, **more):
    closed = sankoff_slow.close_triangle(cost)
    d = dict(name=name, group=group, datatype=datatype, codes=codes, weights=weights, cost=np.ascontiguousarray(cost, dtype=np.uint32),
             sym=bool((closed == closed.T).all()), back=back, ninf=ninf, radii=tuple(radii), nodes=nodes)
    d.update(more)
    return d


A_COUNTS_DNA = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257)
A_COUNTS_OTHER = (1, 33, 64, 129)
A_KINDS = {"dna": (DNA, lambda: random_metric(4, 6)), "aa": (AA, lambda: random_metric(20, 4)),
           "ms32": (GENERIC, lambda: random_metric(32, 5)), "dna_asym": (DNA, lambda: random_asymmetric(4, 11))}


@functools.lru_cache(maxsize=None)
def case_a(kind, ninf):
    """group A: 9 taxa, random topology, exactly ninf informative patterns"""
    dt, mk = A_KINDS[kind]
    codes, w, _kept = edge_alignment(9, ninf, dt, 1000 + ninf)
    return _case(f"A-{kind}-{ninf}", "A", dt, codes, w, mk(), trees.random_topology(9, np.random.default_rng(ninf)), ninf=ninf, radii=(3,))


A_PARAMS = [("dna", k) for k in A_COUNTS_DNA] + [(kind, k) for kind in ("aa", "ms32", "dna_asym") for k in A_COUNTS_OTHER]
B_PARAMS = [(n, kind) for n in (4, 5, 6) for kind in ("dna", "dna_asym", "aa", "aa_asym")]


@functools.lru_cache(maxsize=None)
def case_b(n, kind):
    """group B: 4, 5 and 6 taxa, radii 1 and 6 (clipped to ntips - 3 by the scan)"""
    dt = DNA if kind.startswith("dna") else AA
    S = STATES[dt]
    cost = random_asymmetric(S, 20 + n) if kind.endswith("asym") else random_metric(S, 30 + n)
    codes, w, _kept = edge_alignment(n, 37, dt, 2000 + n)
    return _case(f"B-{kind}-{n}", "B", dt, codes, w, cost, trees.random_topology(n, np.random.default_rng(n)), ninf=37, radii=(1, 6),
                 every_tree=all_topologies(n))


C_PARAMS = ("caterpillar128_dna", "caterpillar64_aa", "balanced64_dna_asym")


@functools.lru_cache(maxsize=None)
def case_c(which):
    """group C: the deepest and the flattest trees; radius 6 in registers, radius 13 in k_snk_scan_deep, 12 spread prune nodes"""
    if which == "caterpillar128_dna":
        codes, w, _ = edge_alignment(128, 96, DNA, 31)
        return _case("C-" + which, "C", DNA, codes, w, random_metric(4, 6), caterpillar(128), ninf=96, radii=(6, 13), nodes=12)
    if which == "caterpillar64_aa":
        codes, w, _ = edge_alignment(64, 40, AA, 32)
        return _case("C-" + which, "C", AA, codes, w, random_metric(20, 4), caterpillar(64), ninf=40, radii=(6, 13), nodes=12)
    codes, w, _ = edge_alignment(64, 96, DNA, 33)
    return _case("C-" + which, "C", DNA, codes, w, random_asymmetric(4, 11), balanced(64), ninf=96, radii=(6, 13), nodes=12)


# group D: (name, data type, taxa, largest closed entry on the packed side -- one more is past the gate)
D_GATES = {"aa20": (AA, 20, 1091), "dna9": (DNA, 9, 2426), "bin9": (BIN, 9, 2425)}
D_PARAMS = [(g, m) for g in D_GATES for m in ("unit", "metric")]


@functools.lru_cache(maxsize=None)
def case_d(gate, matrix, over):
    """group D: the caller's matrix has `largest + over` as its largest entry (over = 0: the last one the 16-bit store takes, 1: the
    first one it does not).  Binary data: the two rows the 4-row kernels add are filled with largest + 1, so the gate sits one lower
    than 3 n (largest + 1) < 2^16 says.  Columns: 12 in which the taxa differ as far as the alphabet allows (a view entry grows by a
    full cost per tip), then random ones."""
    dt, n, largest = D_GATES[gate]
    S = STATES[dt]
    big = largest + over
    if matrix == "unit" or S == 2:
        cost = unit_cost(S, big)
        if S == 2 and matrix == "metric":
            cost[1, 0] = big - 3                                  # (2 x 2: any matrix is closed; this one is not symmetric)
    else:
        cost = metric_with_largest(S, big, 7)
    codes, w, _ = edge_alignment(n, 40, dt, 4000 + n, all_different=12)
    w = np.minimum(w, 9).astype(np.int32)                         # (totals of 40 patterns x 20 000 stay far inside 32 bits)
    return _case(f"D-{gate}-{matrix}-{'over' if over else 'under'}", "D", dt, codes, w, cost,
                 trees.random_topology(n, np.random.default_rng(n + 1)), ninf=40, radii=(6,), nodes=8)


# The levels a scan reaches decide its kernel: k_snk_scan keeps 12 (DNA) or 6 (20 and 32 states), k_snk_scan_deep takes what is deeper.
# dna_ambig (14 taxa: depth 8 at most) and aa (11 taxa: depth 6 at most) stay in the register kernel at any radius; morph32_40,
# dna_48 (the one DNA fixture whose tree does not clip radius 13) and the protein caterpillar of group C ("cat64_aa": no fixture has a
# protein tree deeper than 6 levels) reach the deep kernel -- `deep` says which, and the GPU test asserts it from what was dispatched.
E_DEEP = ("morph32_40", "dna_48", "cat64_aa")
E_PARAMS = [(name, kind) for name in ("dna_ambig", "aa", "morph32_40", "dna_48", "cat64_aa") for kind in ("sym", "asym")]


@functools.lru_cache(maxsize=None)
def case_e(name, kind):
    """group E: the golden fixtures the wide-address scan runs on (and group C's protein caterpillar)"""
    if name == "cat64_aa":
        c = case_c("caterpillar64_aa")
        cost = random_asymmetric(20, 11) if kind == "asym" else random_metric(20, 4)
        # (scans only: group C climbs away from this tree)
        return _case(f"E-{name}-{kind}", "E", AA, c["codes"], c["weights"], cost, c["back"], ninf=40, radii=(6, 13), nodes=6,
                     slow_radii=(6,), slow_nodes=2, climb=False, ras=False, deep=True)
    fx = load_fixture(name)
    S = fx["S"] if fx["datatype"] != GENERIC else 32
    cost = random_asymmetric(S, 11) if kind == "asym" else random_metric(S, 4)
    big = name in ("morph32_40", "dna_48")                      # (the CPU check of the plain reference walks fewer candidates there)
    # (32 states on 40 taxa: the first 129 of the 360 columns -- the oracle's climb is what such a case spends its time in)
    cols = slice(0, 129) if name == "morph32_40" else slice(None)
    return _case(f"E-{name}-{kind}", "E", fx["datatype"], np.ascontiguousarray(fx["codes_np"][:, cols]), fx["weights_np"][cols].copy(), cost,
                 np.array(fx["spr"]["start_back"], dtype=np.int32), radii=(6, 13), nodes=6, slow_radii=(6,) if big else (6, 13),
                 slow_nodes=2 if big else 6, deep=name in E_DEEP,
                 # (40 and 48 taxa: the climb starts from the reference climb's final tree, a few moves from its end under these costs)
                 **({"climb_back": np.array(fx["spr"]["final_back"], dtype=np.int32), "ras": False} if big else {}))


def f_weight_vectors(P):
    """group F: ones -> zeros and heavy ones -> ones again"""
    rng = np.random.default_rng(5)
    heavy = np.zeros(P, dtype=np.int32)
    heavy[rng.permutation(P)[:max(6, P // 3)]] = rng.choice([1, 7, 65535, 100000, 40000, 3], size=max(6, P // 3))
    ones = np.ones(P, dtype=np.int32)
    return [ones, heavy, ones.copy()]


F_PARAMS = ("dna", "aa")


@functools.lru_cache(maxsize=None)
def case_f(kind):
    dt = DNA if kind == "dna" else AA
    codes, _w, _ = edge_alignment(12, 70, dt, 77)
    P = codes.shape[1]
    cost = random_metric(STATES[dt], 6)
    return _case(f"F-{kind}", "F", dt, codes, np.ones(P, dtype=np.int32), cost, trees.random_topology(12, np.random.default_rng(8)),
                 ninf=70, radii=(6,), nodes=1, weight_vectors=f_weight_vectors(P))


def case_f_empty():
    """no informative pattern under a cost matrix: ninf = 0, one row of 32 padded patterns"""
    codes = np.full((6, 10), 1, dtype=np.uint8)
    codes[0, :] = 15
    return _case("F-empty", "F", DNA, codes, np.ones(10, dtype=np.int32), random_metric(4, 6),
                 trees.random_topology(6, np.random.default_rng(1)), ninf=0, radii=(6,))


# every input of groups A-F by key (the CPU test walks this list; a case is built when it is asked for)
CASE_KEYS = ([("A",) + p for p in A_PARAMS] + [("B",) + p for p in B_PARAMS] + [("C", p) for p in C_PARAMS]
             + [("D", g, m, over) for g, m in D_PARAMS for over in (0, 1)] + [("E",) + p for p in E_PARAMS]
             + [("F", p) for p in F_PARAMS] + [("F0",)])


def get_case(key):
    return {"A": case_a, "B": case_b, "C": case_c, "D": case_d, "E": case_e, "F": case_f, "F0": case_f_empty}[key[0]](*key[1:])


def spread(order, k):
    """k prune nodes spread over the oracle's node order (all of them for k = 0)"""
    order = [int(r) for r in order]
    if k == 0 or k >= len(order):
        return order
    return [order[(i * len(order)) // k] for i in range(k)]


# ---- the plain reference's answers, computed once per case and shared
@functools.lru_cache(maxsize=None)
def _slow_memo(name):
    return {}


def slow_tree(case, back=None, weights=None, root_rec=None):
    """(score, per-pattern lengths [P]) of sankoff_slow at the edge of tip 1 (or rooted at record root_rec, the subtree behind it in
    the leaf's place); cached per (case, tree, weights, root)"""
    memo = _slow_memo(case["name"])
    b = case["back"] if back is None else back
    w = case["weights"] if weights is None else weights
    key = (np.asarray(b, dtype=np.int32).tobytes(), np.asarray(w, dtype=np.int32).tobytes(), root_rec)
    if key not in memo:
        memo[key] = sankoff_slow.tree_cost(case["codes"], w, b, case["cost"], case["datatype"], root_rec=root_rec)
    return memo[key]


def slow_candidate(case, prune, q, back=None, weights=None):
    """length of the tree after pruning at record `prune` and regrafting on the branch of record q.  A symmetric matrix: the length
    does not depend on the root, it is taken at tip 1.  Any other: the insertion test evaluates at the new node's edge towards the far
    end back[q] of the branch, the far side being the parent side (testInsertParsimony's evaluateParsimony(p->next->next))."""
    b = case["back"] if back is None else back
    prune = int(prune)
    moved = sankoff_slow.apply_spr(b, prune, int(q))
    nn = 3 * (prune // 3) + (prune % 3 + 2) % 3
    return slow_tree(case, moved, weights, None if case["sym"] else nn)[0]
