"""CPU checks of the polytomy witnesses (tests/polytomy_witness.py): the two agree with each other, with the branch-length witness
on fully resolved trees and with a golden fixture's score; hand cases that pin the rule; the validator's cases.  No GPU."""
import numpy as np
import pytest

import brlen_witness as bw
import nni_snk_cases as cases
import polytomy_witness as pw
from helpers import load_fixture, topology_splits
from nni_snk_witness import SnkScorer


def _alignment(n, P, protein, seed):
    rng = np.random.default_rng(seed)
    if protein:
        codes = rng.integers(0, 20, size=(n, P))
        odd = rng.integers(20, 23, size=(n, P))
    else:
        codes = 1 << rng.integers(0, 4, size=(n, P))
        odd = rng.integers(1, 16, size=(n, P))
    codes = np.where(rng.random((n, P)) < 0.1, odd, codes).astype(np.uint8)
    return codes, rng.integers(1, 6, size=P).astype(np.int32)


def _dna(rows):
    return np.array([[{"A": 1, "C": 2, "G": 4, "T": 8}[c] for c in r] for r in rows], dtype=np.uint8)


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_the_two_witnesses_agree_on_random_collapses(protein):
    from mpboot_amd import trees
    dt = 1 if protein else 0
    for n, P, frac, seed in ((4, 9, 1.0, 0), (5, 9, 0.5, 1), (6, 7, 0.5, 2), (9, 6, 0.4, 3), (12, 5, 0.7, 4)):
        codes, weights = _alignment(n, P, protein, seed)
        rng = np.random.default_rng(seed)
        first, nbr = pw.random_collapse(trees.random_topology(n, rng), n, rng, frac)
        assert pw.validate(first, nbr, n) is None
        for root in (1, n):
            w = pw.PolyWitness(codes, weights, dt)
            length, ptn = w.parsimony(first, nbr, root)
            order, subst = w.substitutions(first, nbr, root)
            r_len, r_ptn, r_order, r_subst = pw.recursive_fitch(codes, weights, dt, first, nbr, root)
            assert len(order) == n + len(first) - 2 and order == r_order
            assert length == r_len and ptn.tolist() == r_ptn and subst.tolist() == r_subst
            if n <= 6 or not protein:
                cost = cases.cost_of("asym" if root == 1 else "metric", 20 if protein else 4, seed=seed + 1)
                w = pw.PolyWitness(codes, weights, dt, cost=cost)
                length, ptn = w.parsimony(first, nbr, root)
                order, subst = w.substitutions(first, nbr, root)
                r_len, r_ptn, r_order, r_subst = pw.recursive_weighted(codes, weights, dt, cost, first, nbr, root)
                assert order == r_order and length == r_len and ptn.tolist() == r_ptn and subst.tolist() == r_subst


@pytest.mark.parametrize("name", ["dna_clean", "aa"])
def test_a_resolved_tree_gives_the_binary_witness_and_the_golden_score(name):
    from mpboot_amd import trees
    fx = load_fixture(name)
    codes, weights, dt = fx["codes_np"], fx["weights_np"], fx["datatype"]
    n = codes.shape[0]
    for t in fx["trees"][:2]:
        back = np.array(t["back"], dtype=np.int32)
        first, nbr = trees.collapse_branches(back, n, ())
        w = pw.PolyWitness(codes, weights, dt, keep=fx["informative"])
        assert w.parsimony(first, nbr, 1)[0] == t["score"]
        for root in (1, n):
            order, subst = w.substitutions(first, nbr, root)
            b_order, b_subst, b_total = bw.fitch_substitutions(codes, weights, dt, back, n, root, keep=fx["informative"])
            assert order == b_order and (subst == b_subst).all() and (b_total == t["score"]).all()
    cost = cases.cost_of("asym", fx["S"])
    back = np.array(fx["trees"][0]["back"], dtype=np.int32)
    first, nbr = trees.collapse_branches(back, n, ())
    sc = SnkScorer(codes, weights, cost, protein=fx["S"] == 20)
    w = pw.PolyWitness(codes, weights, dt, cost=cost)
    for root in (1, n):
        assert w.parsimony(first, nbr, root)[0] == sc.length(back, root)
        order, val = w.substitutions(first, nbr, root)
        b_order, b_val = bw.weighted_values(sc, back, n, root)
        assert order == b_order and (val == b_val).all()


def test_hand_cases():
    one = np.ones(1, dtype=np.int32)
    first, nbr = pw.star(4)
    # the star A, C, G, T rooted at A: the three children share nothing -> ONE step at the node, their union {C, G, T} misses A ->
    # one more at the root edge: 2, where any binary resolution (and a hard polytomy) takes 3
    assert pw.PolyWitness(_dna(["A", "C", "G", "T"]), one, 0).parsimony(first, nbr, 1)[0] == 2
    assert pw.recursive_fitch(_dna(["A", "C", "G", "T"]), one, 0, first, nbr, 1)[0] == 2
    # the star A, A, C, C: children {A, C, C} -> one step, union {A, C} holds the root's A
    assert pw.PolyWitness(_dna(["A", "A", "C", "C"]), one, 0).parsimony(first, nbr, 1)[0] == 1
    # the length changes with the root leaf, on the star A, A, C, C, G:
    codes = _dna(["A", "A", "C", "C", "G"])
    first, nbr = pw.star(5)
    w = pw.PolyWitness(codes, one, 0)
    assert w.parsimony(first, nbr, 1)[0] == 1                        # children A, C, C, G: one step, the union holds A
    assert w.parsimony(first, nbr, 5)[0] == 2                        # children A, A, C, C: one step, the union misses G: another
    assert pw.recursive_fitch(codes, one, 0, first, nbr, 5)[0] == 2
    # weighted, unit costs, the star A, C, G, T: a true Sankoff minimum, 3 whatever the root
    unit = 1 - np.eye(4, dtype=np.int64)
    first, nbr = pw.star(4)
    for root in (1, 4):
        assert pw.PolyWitness(_dna(["A", "C", "G", "T"]), one, 0, cost=unit).parsimony(first, nbr, root)[0] == 3


def test_the_validator_cases():
    assert pw.validate(*pw.GOOD5, 5) is None
    for first, nbr in (pw.star(4), pw.star(65)):
        assert pw.validate(first, nbr, len(nbr)) is None
    for name, n, first, nbr in pw.MALFORMED:
        assert pw.validate(first, nbr, n) is not None, name


def test_collapse_branches_round_trips():
    from mpboot_amd import trees
    for n, seed in ((4, 0), (7, 1), (16, 2), (40, 3)):
        rng = np.random.default_rng(seed)
        back = trees.random_topology(n, rng)
        first, nbr = trees.collapse_branches(back, n, ())
        assert (trees.lists_to_back(first, nbr, n) == back).all()            # nothing contracted: the same tree, slot for slot
        inner = [(v, int(back[3 * v + s]) // 3) for v in range(n + 1, 2 * n - 1) for s in range(3) if int(back[3 * v + s]) // 3 > v]
        assert len(inner) == n - 3
        pick = [br for br in inner if rng.random() < 0.5]
        first, nbr = trees.collapse_branches(back, n, pick)
        assert pw.validate(first, nbr, n) is None
        assert len(first) - 1 == n - 2 - len(pick) and first[-1] == 3 * (n - 2) - 2 * len(pick)
        # its bipartitions are the binary tree's without the contracted ones
        below = {}
        for v1, v2 in reversed(pw.rooted(first, nbr, n, 1)[0]):
            below[v2] = below.get(v2, frozenset()) | (frozenset([v2]) if v2 <= n else frozenset())
            below[v1] = below.get(v1, frozenset()) | below[v2]
        splits = {s for v, s in below.items() if v > n}
        assert len(splits) == len(first) - 1 and splits <= topology_splits(back, n)
        first, nbr = trees.collapse_branches(back, n, inner)                 # everything contracted: the star
        assert len(first) == 2 and sorted(nbr.tolist()) == list(range(1, n + 1))
