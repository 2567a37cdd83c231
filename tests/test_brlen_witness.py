"""CPU checks of the branch-length witness (tests/brlen_witness.py) against the project's other scorers.  No GPU."""
import numpy as np
import pytest

import brlen_witness as bw
import nni_snk_cases as cases
from helpers import FIXTURES, load_fixture
from nni_snk_witness import SnkScorer
from nni_witness import NniWitness
from oracle import iqtree_fitch, pyoracle as po
from oracle import sankoff_slow

ALPHA = {"DNA": ("DNA", 4), "WAG": ("AA", 20), "BIN": ("BIN", 2), "MOR": ("MOR", 32)}


def _random_trees(n, seeds):
    from mpboot_amd import trees
    return [trees.random_topology(n, np.random.default_rng(s)) for s in seeds]


@pytest.mark.parametrize("name", FIXTURES)
def test_every_branch_sees_the_tree_length(name):
    """steps(side 1) + steps(side 2) + subst is the Fitch length of the tree at EVERY branch: over all patterns the slow IQ-TREE
    restatement's and the pinned oracle's with every site kept, over the informative ones the pinned oracle's as it packs them"""
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    alpha, ns = ALPHA[fx["pll_type"]]
    states = iqtree_fitch.convert_states(fx["rows"], alpha)
    freq = fx["weights"] if states.shape[1] == fx["P"] else [1] * states.shape[1]       # (a de-duplicated fixture: its rows are the sites)
    o_all = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], keep_all=True)
    o_inf = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"])
    for root, back in zip((1, n, 2), _random_trees(n, (0, 1, 2))):
        want, _ = iqtree_fitch.compute_parsimony(states, freq, back, ns)
        assert o_all.score_tree(back) == want
        order, subst, total = bw.fitch_substitutions(fx["codes_np"], fx["weights_np"], fx["datatype"], back, n, root)
        assert len(order) == 2 * n - 3 and len({frozenset(b) for b in order}) == 2 * n - 3
        assert (total == want).all()
        assert (subst >= 0).all() and subst.sum() > 0
        _o, fast = bw.fitch_substitutions_fast(fx["codes_np"], fx["weights_np"], fx["datatype"], back, n, root)
        assert (fast == subst).all()
        _o, _s, total_inf = bw.fitch_substitutions(fx["codes_np"], fx["weights_np"], fx["datatype"], back, n, root, keep=fx["informative"])
        assert (total_inf == o_inf.score_tree(back)).all()


@pytest.mark.parametrize("name", ["dna_clean", "dna_48", "aa_40"])
def test_branch_order_is_the_evalnnis_order_on_the_inner_branches(name):
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    for root, back in zip((1, n, 3), _random_trees(n, (0, 1, 2))):
        order = bw.branch_order(back, n, root)
        assert order[0][0] == root
        inner = [(v2, v1) for v1, v2 in order if v1 > n and v2 > n]          # evalNNIs names a branch (node, dad)
        assert inner == NniWitness(back, n, None, root_taxon=root).full_order()
        # every branch from its root side: node1 was met before node2
        seen = {root}
        for v1, v2 in order:
            assert v1 in seen and v2 not in seen
            seen.add(v2)


@pytest.mark.parametrize("name,kind", [("dna_ambig", "tstv"), ("dna_dups", "metric"), ("aa", "metric")])
def test_symmetric_matrix_every_branch_gives_the_tree_length(name, kind):
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    cost = cases.cost_of(kind, fx["S"])
    sc = SnkScorer(fx["codes_np"], fx["weights_np"], cost, protein=fx["S"] == 20)
    for back in _random_trees(n, (0, 1, 2)):
        want = sankoff_slow.tree_cost(fx["codes_np"], fx["weights_np"], back, cost, fx["datatype"])[0]
        for rev in (False, True):
            order, val = bw.weighted_values(sc, back, n, 1, reverse=rev)
            assert len(order) == 2 * n - 3
            assert (val == want).all()


@pytest.mark.parametrize("name", ["dna_ambig", "aa"])
def test_asymmetric_matrix_orientation(name):
    """a matrix that is not symmetric: a pendant branch equals the slow DP rooted at its leaf (whichever end of the branch the leaf
    is), inner branches differ among themselves, and an inner branch differs from its own reversed orientation"""
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    cost = cases.cost_of("asym", fx["S"])
    sc = SnkScorer(fx["codes_np"], fx["weights_np"], cost, protein=fx["S"] == 20)
    differ = reversed_differs = 0
    for root, back in zip((1, n), _random_trees(n, (0, 1))):
        order, val = bw.weighted_values(sc, back, n, root)
        _o, rev = bw.weighted_values(sc, back, n, root, reverse=True)
        inner = []
        for (v1, v2), x, y in zip(order, val, rev):
            leaf = v1 if v1 <= n else (v2 if v2 <= n else 0)
            if leaf:
                assert x == sankoff_slow.tree_cost(fx["codes_np"], fx["weights_np"], back, cost, fx["datatype"], root_tip=leaf)[0]
            else:
                inner.append(int(x))
                reversed_differs += int(x != y)
        differ += int(len(set(inner)) > 1)
    assert differ >= 1 and reversed_differs >= 1


def test_length_formula_rules():
    """the 1 / N rule of a zero count, the uncorrected length where x <= 0, the floor"""
    got = bw.lengths([0, 1, 30, 75, 76, 1000], 100, 4)
    assert got[0] == got[1] == -np.log(1 - (4 / 3) * 0.01) / (4 / 3)
    assert got[2] == -np.log(1 - (4 / 3) * 0.3) / (4 / 3)
    assert got[3] == 0.75 and got[4] == 0.76 and got[5] == 10.0          # x = 0 and x < 0: as observed
    assert bw.lengths([0], 10 ** 7, 4)[0] == 1e-6
    assert bw.lengths([3], 100, 20)[0] == -np.log(1 - (20 / 19) * 0.03) / (20 / 19)
