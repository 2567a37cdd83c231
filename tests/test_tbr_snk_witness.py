"""CPU checks of the weighted TBR witness (tests/tbr_snk_witness.py): its from-scratch form and its vectorised form agree on every
entry, both give oracle/sankoff_slow.py's and polytomy_witness.recursive_weighted's length at EVERY root leaf under a symmetric
matrix, under a matrix that is not symmetric the lengths at different root leaves differ (why such an engine is refused), the
descent walks downhill through valid trees, and the pinned seed is an input on which a weighted SPR-local optimum is not
TBR-local.  No GPU."""
import numpy as np
import pytest

import polytomy_witness as pw
import tbr_snk_witness as ts
import tbr_witness as tw
from mpboot_amd import trees
from nni_snk_cases import cost_of
from oracle import sankoff_slow as slow

STATES = {0: 4, 1: 20, 3: 32}
ALPHABET = {0: "dna", 1: "aa", 3: "m32"}


def _records(n):
    return [3 * t for t in range(1, n + 1)] + [3 * v + s for v in range(n + 1, 2 * n - 1) for s in range(3)]


@pytest.mark.parametrize("n,P,dt,kind", [(4, 9, 0, "tstv"), (5, 12, 0, "metric"), (6, 7, 1, "metric"), (7, 5, 3, "metric"), (8, 30, 0, "tstv"),
                                         (9, 20, 0, "metric")])
def test_the_forms_agree_on_every_entry_of_small_trees(n, P, dt, kind):
    """every record, radii 1, 2, 3 and 255: the vectorised matrix is the from-scratch matrix, [0][0] the tree as it is"""
    codes, w = tw.alignment(n, P, ALPHABET[dt], 10 * n + dt)
    wit = ts.TbrSnkWitness(codes, w, dt, cost_of(kind, STATES[dt], seed=n))
    back = trees.random_topology(n, np.random.default_rng(n))
    length, views = wit.length(back), wit.views(back)
    n_tbr, memo = 0, {}
    for p in _records(n):
        for rad in (1, 2, 3, 255):
            F, G, cost = wit.matrix(back, p, rad, views)
            assert (cost == wit.matrix(back, p, rad)[2]).all()                  # (the parts kept in `views` change nothing)
            # ... nor does the table of subtree rows kept from one edited tree to the next
            assert all(wit.scratch(back, p, f, g, memo) == cost[i, j] for i, f in enumerate([ts.NONE] + F) for j, g in enumerate([ts.NONE] + G))
            assert [(r, d) for r, d in tw.lists(back, n, p, rad)[0]] == list(zip(F, [d for _, d in tw.lists(back, n, p, rad)[0]]))
            assert cost[0, 0] == length and (cost == wit.scratch_matrix(back, p, rad)).all(), (p, rad)
            n_tbr += int((cost[1:, 1:] != length).sum())
    assert n <= 5 or n_tbr > 0                               # true TBR entries were among them


@pytest.mark.parametrize("dt,kind", [(0, "tstv"), (0, "metric"), (1, "metric")])
def test_lengths_equal_the_slow_oracle_and_the_recursion_at_every_root_leaf(dt, kind):
    """the tree as it is and drawn TBR edits of it: one length whatever the root leaf, and the same from three other programmes"""
    n, P = (7, 6) if dt == 1 else (9, 14)
    codes, w = tw.alignment(n, P, ALPHABET[dt], 77 + dt)
    cost = cost_of(kind, STATES[dt])
    wit = ts.TbrSnkWitness(codes, w, dt, cost)
    rng = np.random.default_rng(3)
    back = trees.random_topology(n, rng)
    cases = [back]
    for _ in range(3):
        p = _records(n)[int(rng.integers(4 * n - 6))]
        F, G, mat = wit.matrix(back, p, 255)
        i, j = int(rng.integers(1 + len(F))), int(rng.integers(1 + len(G)))
        new = trees.apply_tbr(back, p, ([ts.NONE] + F)[i], ([ts.NONE] + G)[j])
        trees.validate(new, n)
        assert wit.length(new) == mat[i, j]
        cases.append(new)
    for b in cases:
        first, nbr = trees.back_to_lists(b, n)
        want = wit.length(b)
        for root in range(1, n + 1):
            assert wit.length(b, root) == want
            assert slow.tree_cost(codes, w, b, cost, dt, root_tip=root)[0] == want
            assert pw.recursive_weighted(codes, w, dt, cost, first, nbr, root)[0] == want


def test_under_a_matrix_that_is_not_symmetric_the_root_leaf_matters():
    """the pinned seed: the lengths of ONE tree at its root leaves differ, in the witness's recursion and in the slow oracle alike, so
    an entry of a TBR matrix would depend on an evaluation edge nothing fixes"""
    n, P = 9, 60
    codes, w = tw.alignment(n, P, "dna", 5)
    cost = cost_of("asym", 4, seed=ts.ASYM_SEED)
    wit = ts.TbrSnkWitness(codes, w, 0, cost)
    back = trees.random_topology(n, np.random.default_rng(5))
    mine = [wit.length(back, root) for root in range(1, n + 1)]
    assert mine == [slow.tree_cost(codes, w, back, cost, 0, root_tip=root)[0] for root in range(1, n + 1)]
    assert len(set(mine)) > 1
    sym = ts.TbrSnkWitness(codes, w, 0, cost_of("tstv", 4))
    assert len({sym.length(back, root) for root in range(1, n + 1)}) == 1


def test_the_descent_walks_downhill_through_valid_trees():
    n = 10
    codes, w = tw.alignment(n, 50, "dna", 21)
    wit = ts.TbrSnkWitness(codes, w, 0, cost_of("metric", 4))
    back = trees.random_topology(n, np.random.default_rng(21))
    end, length, moves = wit.descent(back, 255)
    assert moves and [m[3] for m in moves] == sorted({m[3] for m in moves}, reverse=True) and moves[-1][3] == length < wit.length(back)
    trees.validate(end, n)
    assert wit.length(end) == length and min(b[0] for b in wit.sweep_best(end, 255)[0]) >= length
    cur = back
    for rec, f, g, ln in wit.descent(back, 255, max_moves=2)[2]:
        cur = trees.apply_tbr(cur, rec, f, g)
        assert wit.length(cur) == ln
    assert wit.descent(back, 255, max_moves=2)[2] == moves[:2]


def test_a_weighted_spr_local_optimum_is_not_tbr_local_on_the_pinned_seed():
    codes, w, back = ts.noisy_case(ts.PINNED_SEED)
    wit = ts.TbrSnkWitness(codes, w, 0, cost_of("tstv", 4))
    spr_back, spr_len, spr_moves = wit.descent(back, ts.PINNED_RADIUS, spr_only=True)
    assert spr_moves and min(b[0] for b in wit.sweep_best(spr_back, ts.PINNED_RADIUS, spr_only=True)[0]) >= spr_len
    tbr_back, tbr_len, tbr_moves = wit.descent(spr_back, ts.PINNED_RADIUS)
    assert tbr_len < spr_len and tbr_moves and all(f != ts.NONE and g != ts.NONE for _r, f, g, _l in tbr_moves[:1])
    assert wit.length(tbr_back) == tbr_len
