"""The witness of the weighted NNI climb (tests/nni_snk_witness.py) against the project's two other Sankoff implementations, and
the committed GPU cases (tests/nni_snk_cases.py) against what they are there to exercise.  No GPU."""
import numpy as np
import pytest

import nni_snk_cases as cases
from helpers import load_fixture
from nni_snk_witness import SnkNniWitness, SnkScorer
from oracle import pyoracle as po
from oracle import sankoff_slow


def _random_trees(n, seeds):
    from mpboot_amd import trees
    return [trees.random_topology(n, np.random.default_rng(s)) for s in seeds]


def _inner_branches(back, n):
    return SnkNniWitness(back, n, None).full_order()


@pytest.mark.parametrize("name,kind", [("dna_ambig", "tstv"), ("dna_dups", "metric"), ("aa", "metric")])
def test_symmetric_matrix_every_inner_branch_gives_the_tree_length(name, kind):
    """a symmetric matrix: the length does not depend on the root edge, so the edge-rooted scorer must give, at EVERY inner branch
    and in both orientations, what the slow DP and the pinned oracle give for the tree"""
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    cost = cases.cost_of(kind, fx["S"])
    sc = SnkScorer(fx["codes_np"], fx["weights_np"], cost, protein=fx["S"] == 20)
    o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
    for back in _random_trees(n, (0, 1, 2)):
        want = sankoff_slow.tree_cost(fx["codes_np"], fx["weights_np"], back, cost, fx["datatype"])[0]
        assert o.score_tree(back) == want
        br = _inner_branches(back, n)
        assert len(br) == n - 3
        for v1, v2 in br:
            assert sc.edge_length(back, v1, v2) == want
            assert sc.edge_length(back, v2, v1) == want
        assert sc.length(back, 1) == want and sc.length(back, n) == want


@pytest.mark.parametrize("name", ["dna_ambig", "aa"])
def test_asymmetric_matrix_pendant_edges_equal_the_slow_dp_rooted_there(name):
    """a matrix that is not symmetric: at the pendant edge of tip t (t the node1 side, the rest of the tree the parent) the scorer
    equals the slow DP rooted at t -- and the lengths do differ between root edges"""
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    cost = cases.cost_of("asym", fx["S"])
    assert (sankoff_slow.close_triangle(cost) == cost).all()
    sc = SnkScorer(fx["codes_np"], fx["weights_np"], cost, protein=fx["S"] == 20)
    seen = set()
    for back in _random_trees(n, (0, 1)):
        for t in range(1, n + 1):
            want = sankoff_slow.tree_cost(fx["codes_np"], fx["weights_np"], back, cost, fx["datatype"], root_tip=t)[0]
            assert sc.edge_length(back, t, int(back[3 * t]) // 3) == want
            assert sc.length(back, t) == want
            seen.add(want)
    assert len(seen) > 2


@pytest.fixture(scope="module")
def climbs():
    return {(c["id"], sp): cases.witness(c, sp) for c in cases.CASES for sp in (True, False)}


def test_cases_take_the_kept_worse_step(climbs):
    kept = {cid for (cid, _sp), w in climbs.items() if w.kept_worse > 0}
    assert len(kept) >= 2
    # ... under a symmetric matrix too (several NNIs at once are not additive), not only where the root edge matters
    assert any(c["cost"] != "asym" and c["id"] in kept for c in cases.CASES)
    for w in climbs.values():
        assert w.rollbacks == 0


def test_cases_apply_several_nnis_in_one_step(climbs):
    assert any(w.most_applied >= 2 for w in climbs.values())


def test_cases_end_at_the_step_cap_and_before_it(climbs):
    by_id = {c["id"]: c for c in cases.CASES}
    capped = [cid for (cid, _sp), w in climbs.items() if w.result[2] == by_id[cid]["steps"] + 1]
    assert capped and any(by_id[cid]["steps"] < 50 for cid in capped)
    assert any(w.result[2] <= by_id[cid]["steps"] for (cid, _sp), w in climbs.items())


def test_final_tree_is_the_start_tree_with_the_log_replayed(climbs):
    for (cid, _sp), w in climbs.items():
        case = next(c for c in cases.CASES if c["id"] == cid)
        _fx, _cost, n, root, back, sc = cases.setup(case)
        r = SnkNniWitness(back, n, sc, root_taxon=root)
        for mv in w.log:
            r.swap(mv)
        assert (r.back == w.back).all()
        assert sc.length(w.back, root) == w.result[0]
