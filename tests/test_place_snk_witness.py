"""CPU checks of the weighted taxon-insertion witness (tests/place_snk_witness.py): its forms agree with one another and with
polytomy_witness.recursive_weighted(completed tree, root = query), the orientation is exercised by a matrix that is not symmetric,
and on small complete trees every entry is oracle/sankoff_slow.py's length of the completed tree rooted at the query's edge.  No GPU."""
import numpy as np
import pytest

import place_snk_witness as psw
import place_witness as plw
import polytomy_witness as pw
from nni_snk_cases import cost_of

KINDS = {0: ("tstv", "metric", "asym"), 1: ("metric", "asym")}


def _alignment(n, P, dt, seed):
    """random tip codes with ambiguity and unknowns, weights 1 .. 5"""
    rng = np.random.default_rng(seed)
    if dt == 1:
        codes, odd = rng.integers(0, 20, size=(n, P)), rng.integers(20, 23, size=(n, P))
    else:
        codes, odd = 1 << rng.integers(0, 4, size=(n, P)), rng.integers(1, 16, size=(n, P))
    codes = np.where(rng.random((n, P)) < 0.25, odd, codes).astype(np.uint8)
    codes[0, 0], codes[1, 1] = (22, 20) if dt == 1 else (15, 5)                   # an unknown and an ambiguity in every input
    return codes, rng.integers(1, 6, size=P).astype(np.int32)


@pytest.mark.parametrize("n", [4, 5, 6, 9])
@pytest.mark.parametrize("dt", [0, 1], ids=["dna", "aa"])
def test_the_forms_agree(dt, n):
    """from scratch (numpy), per pattern (recursive, plain integers) and vectorised; backbones of 3 .. n - 1 tips, every absent taxon
    a query, every root at n <= 6"""
    S = 20 if dt == 1 else 4
    P = 5 if dt == 1 else 9
    codes, weights = _alignment(n, P, dt, 10 * n + dt)
    assert (codes >= (20 if dt == 1 else 5)).any() and (codes == (22 if dt == 1 else 15)).any()      # ambiguity and unknowns are there
    oriented = 0
    for kind in KINDS[dt]:
        cost = cost_of(kind, S)
        wit = psw.SnkPlaceWitness(codes, weights, dt, cost)
        rng = np.random.default_rng(n + len(kind))
        for m in range(3, n):
            tips = rng.permutation(n)[:m] + 1
            first, nbr = plw.backbone(n, tips, rng)
            rest = [t for t in range(1, n + 1) if t not in tips.tolist()]
            for root in (tips.tolist() if n <= 6 else [int(tips[0])]):
                br, cost_s = wit.costs(first, nbr, rest, root)
                vbr, cost_v, vlen = wit.view_costs(first, nbr, rest, root)
                assert br == vbr == plw.walk(first, nbr, n, root) and len(br) == 2 * m - 3
                assert (cost_s == cost_v).all() and vlen == wit.length(first, nbr, root)
                assert (wit.costs(first, nbr, rest, root, reuse=True)[1] == cost_s).all()      # the subtree-row table changes nothing
                assert vlen == psw.recursive_length(codes, weights, dt, cost, first, nbr, root)
                for qi, q in enumerate(rest):
                    for bi, (a, b) in enumerate(br):
                        done = plw.grow(first, nbr, n, q, a, b)
                        assert cost_s[qi, bi] == psw.recursive_length(codes, weights, dt, cost, *done, q), (kind, m, root, q, a, b)
                        if kind == "asym":
                            oriented += cost_s[qi, bi] != psw.recursive_length(codes, weights, dt, cost, *done, root)
                # ... which is recursive_weighted at root = query: one completed tree per backbone in full
                q, (a, b) = rest[0], br[-1]
                done = plw.grow(first, nbr, n, q, a, b)
                assert cost_s[0, -1] == pw.recursive_weighted(codes, weights, dt, cost, *done, root=q)[0]
    # a matrix that is not symmetric: the length at the query's edge is not the length at the backbone's root leaf
    assert oriented > 0


@pytest.mark.parametrize("dt,kind", [(0, "tstv"), (0, "asym"), (1, "metric"), (1, "asym")])
def test_every_entry_is_the_slow_oracles_length_at_the_querys_edge(dt, kind):
    """oracle/sankoff_slow.tree_cost(back, root_tip = t) of the complete tree, t dropped and attached to every branch"""
    from mpboot_amd import trees
    from oracle import sankoff_slow as ss
    n, P, S = 7, 12, 20 if dt == 1 else 4
    codes, weights = _alignment(n, P, dt, 3 + dt)
    cost = cost_of(kind, S)
    wit = psw.SnkPlaceWitness(codes, weights, dt, cost)
    rng = np.random.default_rng(2)
    back = trees.random_topology(n, rng)
    differs = 0
    for t in (int(rng.integers(2, n + 1)), 1):
        root = 1 if t != 1 else 2
        first, nbr = trees.drop_tips(back, n, [t])
        br, got = wit.costs(first, nbr, [t], root)
        assert (wit.view_costs(first, nbr, [t], root)[1] == got).all()
        for i, (a, b) in enumerate(br):
            done = trees.lists_to_back(*trees.insert_tip(first, nbr, n, t, a, b), n)
            assert int(got[0, i]) == ss.tree_cost(codes, weights, done, cost, dt, root_tip=t)[0], (t, a, b)
            differs += int(got[0, i]) != ss.tree_cost(codes, weights, done, cost, dt, root_tip=root)[0]
        assert ss.tree_cost(codes, weights, back, cost, dt, root_tip=t)[0] in got[0].tolist()
    assert (differs > 0) == (kind == "asym")


def test_stepwise_and_the_32_state_alphabet():
    """the stepwise form by both row forms; the last length is the final tree's length at the last taxon's edge; 32 states"""
    rng = np.random.default_rng(1)
    for n, dt, kind in ((6, 0, "tstv"), (9, 0, "asym"), (6, 1, "asym"), (6, 3, "metric")):
        S = psw.STATES[dt]
        if dt == 3:
            codes = np.where(rng.random((n, 7)) < 0.2, 32, rng.integers(0, 32, size=(n, 7))).astype(np.uint8)
            weights = rng.integers(1, 6, size=7).astype(np.int32)
        else:
            codes, weights = _alignment(n, 7, dt, n)
        wit = psw.SnkPlaceWitness(codes, weights, dt, cost_of(kind, S))
        order = (rng.permutation(n) + 1).tolist()
        first, nbr, lengths = psw.stepwise(wit, order)
        assert (first, nbr, lengths) == psw.stepwise(wit, order, scratch=False)
        assert len(lengths) == n - 2 and plw.check(first, nbr, n, order[0]) == "ok" and nbr[-3] == order[-1]
        assert lengths[-1] == wit.length(first, nbr, order[-1])
        assert lengths[0] == wit.length([0, 3], order[:3], order[0])
    # a weight of zero and a pattern not kept change nothing
    codes, weights = _alignment(6, 9, 0, 5)
    keep = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1])
    a = psw.SnkPlaceWitness(codes, weights, 0, cost_of("asym", 4), keep=keep)
    b = psw.SnkPlaceWitness(codes[:, keep != 0], weights[keep != 0], 0, cost_of("asym", 4))
    first, nbr = plw.backbone(6, [1, 2, 3, 4], rng)
    assert (a.view_costs(first, nbr, [5, 6], 1)[1] == b.view_costs(first, nbr, [5, 6], 1)[1]).all()
