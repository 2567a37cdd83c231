"""Sankoff (weighted parsimony) mode of the oracle.

The C++ layer that holds the reference's Sankoff code cannot be built from its sources alone, so there is no
reference run to pin against (parity status of this mode: unpinned).  What is checked:
  * with unit costs it must reproduce the PINNED Fitch oracle exactly (the reference's own claim: `-cost e`
    gives the identical trajectory and score), on every fixture;
  * with other cost matrices it must agree with an independent from-scratch Sankoff DP (oracle/sankoff_slow.py).
"""
import numpy as np
import pytest

import sankoff_edge_cases as sec
from helpers import FIXTURES, load_fixture, trace_tokens
from oracle import pyoracle as po, sankoff_slow


def unit_cost(S):
    return (1 - np.eye(S, dtype=np.uint32)).astype(np.uint32)


def tstv_cost():
    c = np.full((4, 4), 2, dtype=np.uint32)          # A C G T: transitions A<->G, C<->T cost 1
    np.fill_diagonal(c, 0)
    c[0, 2] = c[2, 0] = c[1, 3] = c[3, 1] = 1
    return c


def random_metric(S, seed):
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, 12, size=(S, 3))
    c = np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2).astype(np.uint32)   # L1 distances: a metric
    c[c == 0] = 1
    np.fill_diagonal(c, 0)
    return c


@pytest.fixture(scope="module", params=FIXTURES)
def fx(request):
    return load_fixture(request.param)


def test_unit_costs_reproduce_fitch(fx):
    S = fx["S"]
    f = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"])
    s = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=unit_cost(S))
    f.enable_persite(True)
    for t in fx["trees"][:4]:
        b = np.array(t["back"], dtype=np.int32)
        assert s.score_tree(b) == f.score_tree(b) == t["score"]
        assert (s.pattern_scores()[0] == f.pattern_scores()[0]).all()
    sc = fx["scan"][0]
    back = np.array(sc["back"], dtype=np.int32)
    for o in (f, s):
        o.reset_nodep()
        o.set_tree(back)
        o.score_tree()
        o.seed_ties(po.TIE_RANDOM, 3)
    for rec in sc["order"]:
        toks = []
        for o in (f, s):
            o.set_best(sc["score"])
            o.trace(True)
            o.rearrange(rec, 1, 6)
            toks.append(trace_tokens(*o.get_trace()))
        assert toks[0] == toks[1]


def test_unit_costs_same_trajectories(fx):
    S = fx["S"]
    start = np.array(fx["spr"]["start_back"], dtype=np.int32)
    res = []
    for cost in (None, unit_cost(S)):
        o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
        o.set_tree(start)
        o.seed_ties(po.TIE_RANDOM, 11)
        o.trace(True)
        sc = o.optimize_spr(1, 6)
        res.append((sc, [x.tolist() for x in o.get_moves()], o.get_tree().tolist()))
        o2 = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
        o2.seed_ties(po.TIE_RANDOM, 5)
        res[-1] += (o2.make_tree(42, 3)[0], o2.get_tree().tolist())
    assert res[0] == res[1]


@pytest.mark.parametrize("name", ["dna_ambig", "dna_dups", "aa"])
def test_general_costs_against_slow_dp(name):
    fx = load_fixture(name)
    cost = tstv_cost() if fx["datatype"] == 0 else random_metric(20, 4)
    o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
    for t in fx["trees"][:3]:
        b = np.array(t["back"], dtype=np.int32)
        ref, ptn = sankoff_slow.tree_cost(fx["codes_np"], fx["weights"], b, cost, fx["datatype"])
        assert o.score_tree(b) == ref
        got, total = o.pattern_scores()
        assert total == ref
        inf = o.informative().astype(bool)
        assert (got[inf] == ptn[inf]).all()
    # insertion tests: every traced mp equals the from-scratch cost of the rearranged tree
    back = np.array(fx["scan"][0]["back"], dtype=np.int32)
    o.reset_nodep()
    o.set_tree(back)
    cur = o.score_tree()
    o.seed_ties(po.TIE_RANDOM, 2)
    order = o.nodep()[1:2 * o.n - 1]
    checked = 0
    for rec in order[::5]:
        o.set_best(cur)
        o.trace(True)
        o.rearrange(int(rec), 1, 4)
        q, mp = o.get_trace()
        prune = int(rec)
        for a, m in zip(q, mp):
            if a == -1:
                prune = int(rec)
            elif a == -2:
                prune = int(back[rec])
            elif checked < 60:
                moved = sankoff_slow.apply_spr(back, prune, int(a))
                assert sankoff_slow.tree_cost(fx["codes_np"], fx["weights"], moved, cost, fx["datatype"])[0] == int(m)
                checked += 1
    assert checked > 20


# ---- the inputs of tests/test_gpu_sankoff_edges.py (groups A-F, tests/sankoff_edge_cases.py): oracle and plain reference agree on
#      every one of them, so the reference side of the GPU tests is sound before anything runs on a device
#      (large group E cases: 2 of the 6 scanned prune nodes at radius 6 -- the GPU test compares group E with the oracle alone)
def _oracle(case, weights=None):
    return po.Oracle(case["codes"], case["weights"] if weights is None else weights, datatype=case["datatype"], cost=case["cost"])


def _check_tree(o, case, back, weights=None):
    ref, ptn = sec.slow_tree(case, back, weights)
    assert o.score_tree(back) == ref
    got, total = o.pattern_scores()
    inf = o.informative().astype(bool)
    assert total == ref and (got[inf] == ptn[inf]).all() and not got[~inf].any()
    return ref


def _check_scans(o, case, back, cur, radius, weights=None, nodes=None):
    """every candidate of the chosen prune nodes: the oracle's traced length == the plain reference's length of the rearranged tree.
    A matrix that is not symmetric: the plain reference roots the rearranged tree where the insertion test does (sec.slow_candidate)."""
    o.reset_nodep()
    o.set_tree(back)
    assert o.score_tree() == cur
    o.seed_ties(po.TIE_RANDOM, 2)
    n = case["codes"].shape[0]
    checked = 0
    for rec in sec.spread(o.nodep()[1:2 * n - 1], case["nodes"] if nodes is None else nodes):
        o.set_best(cur)
        o.trace(True)
        o.rearrange(rec, 1, radius)
        prune = rec
        for a, m in zip(*o.get_trace()):
            if a == -1:
                prune = rec
            elif a == -2:
                prune = int(back[rec])
            else:
                assert sec.slow_candidate(case, prune, int(a), back, weights) == int(m), (case["name"], prune, int(a))
                checked += 1
    return checked


@pytest.mark.parametrize("key", sec.CASE_KEYS, ids=["-".join(str(x) for x in k) for k in sec.CASE_KEYS])
def test_edge_case_inputs_against_slow_dp(key):
    case = sec.get_case(key)
    o = _oracle(case)
    if case["ninf"] is not None:
        assert o.num_informative == case["ninf"]
    n = case["codes"].shape[0]
    cur = _check_tree(o, case, case["back"])
    for b in case.get("every_tree", ()):
        _check_tree(o, case, b)
    checked = sum(_check_scans(o, case, case["back"], cur, r, nodes=case.get("slow_nodes")) for r in case.get("slow_radii", case["radii"]))
    assert checked > 0 or case["ninf"] == 0
    for w in case.get("weight_vectors", ()):
        o.set_weights(w)
        cw = _check_tree(o, case, case["back"], w)
        assert _check_scans(o, case, case["back"], cw, 6, w) > 0


@pytest.mark.parametrize("gate,matrix", sec.D_PARAMS)
def test_largest_stored_value_inside_the_16_bit_gate(gate, matrix):
    """what the packed side of each group D case stores: the largest entry of any directed view or transform, and the largest sum of
    three transforms, over the start tree and every rearrangement of the 8 scanned prune nodes at radius 6 -- both below 2^16, and
    the view entries below 2^15 (about n x the largest closed entry)"""
    case = sec.case_d(gate, matrix, 0)
    n = case["codes"].shape[0]
    packed, highest = sec.expect_packed(case["cost"], case["datatype"], n)
    assert packed and not sec.expect_packed(sec.case_d(gate, matrix, 1)["cost"], case["datatype"], n)[0]
    o = _oracle(case)
    o.reset_nodep()
    o.set_tree(case["back"])
    cur = o.score_tree()
    moves = []
    for rec in sec.spread(o.nodep()[1:2 * n - 1], case["nodes"]):
        o.set_best(cur)
        o.trace(True)
        o.rearrange(rec, 1, 6)
        prune = rec
        for a in o.get_trace()[0]:
            prune = rec if a == -1 else int(case["back"][rec]) if a == -2 else prune
            if a >= 0:
                moves.append((prune, int(a)))
    # (on the matrix and the rows the kernels carry: binary codes 1, 2, 3 are DNA codes of the 4-row kernels, the two added rows filled)
    top_view, top_sum = sankoff_slow.largest_entries(case["codes"], case["back"], sec.closed_kernel_matrix(case["cost"], case["datatype"]),
                                                     sankoff_slow.DNA if case["datatype"] == sec.BIN else case["datatype"], moves)
    print(f"\n{case['name']}: largest view entry {top_view}, largest sum of three {top_sum}, n x highest_cost {n * highest}")
    assert top_view <= n * highest < 32768 and top_view < 32768
    assert top_sum < 3 * n * highest < 65536
