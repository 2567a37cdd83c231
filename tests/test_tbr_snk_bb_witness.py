"""CPU checks of the weighted tracked TBR sweep's witness (tests/tbr_snk_bb_witness.py): every row's weighted sum is the entry's
length; under a symmetric matrix the current tree's row is the same at every root leaf and is every visit's [0][0] row of the
vectorised form; under unit costs rows and books are the Fitch witness's; the vectorised form (tests/tbr_snk_bb_cases.py:FormB), which
the one large GPU shape is compared with, gives form (a)'s rows and books; and the inputs the GPU tests use really exercise the
tracker's update rule, so that no GPU test can pass on a run that booked nothing."""
import numpy as np
import pytest

import tbr_witness as tw
from mpboot_amd import trees
from tbr_bb_cases import boot_samples
from tbr_bb_cases import make as make_fitch
from tbr_snk_bb_cases import BIG, CASES, DT, STATES, FormB, make, matrix_of, run, setup, shows_the_rule, visit_rows
from tbr_snk_bb_witness import RowScorer


def _state(w):
    return (w.treels_logl, w.boot_logl, w.boot_counts, w.boot_trees, [sorted(s) for s in w.boot_sets], w.boot_tree_orig_logl,
            w.ufb_draws, int(w.rng.state), w.calls, w.took)


@pytest.mark.parametrize("alphabet,n,P", [("dna", 12, 70), ("aa", 9, 41), ("m32", 8, 23)])
def test_rows_sum_to_lengths_and_do_not_depend_on_the_root_leaf(alphabet, n, P):
    """every entry of every visit at radius 2 and 255: form (a)'s row, taken at three root leaves for the current tree and at leaf 1
    for the joined trees, sums to the entry's length and equals form (b)'s row; [0][0] of every visit is the current tree's row"""
    codes, weights = tw.alignment(n, P, alphabet, 77)
    cost = matrix_of(alphabet)
    back = trees.random_topology(n, np.random.default_rng(5))
    sc = RowScorer(codes, weights, DT[alphabet], cost)
    length, row = sc.length_and_row(back, 1)
    assert int(row @ weights) == length
    for leaf in (2, n // 2 + 1, n):
        other_len, other_row = sc.length_and_row(back, leaf)
        assert other_len == length and (other_row == row).all(), leaf
    views, memo, entries = sc.views(back), {}, 0
    for radius in (2, 255):
        for p in tw.node_order(back, n):
            F, G, rows = visit_rows(sc, back, p, radius, views)
            _F, _G, want_cost = sc.matrix(back, p, radius, views)
            assert (rows[0, 0] == row).all(), (radius, p)
            for i, f in enumerate([tw.NONE] + F):
                for j, g in enumerate([tw.NONE] + G):
                    ln, r = sc.length_and_row(trees.apply_tbr(back, p, f, g), 1, memo)
                    assert (r == rows[i, j]).all() and int(r @ weights) == ln == want_cost[i, j], (radius, p, i, j)
                    entries += 1
    assert entries > 150


@pytest.mark.parametrize("alphabet", ["dna", "aa", "m32"])
@pytest.mark.parametrize("rule", ["default", "cut"])
def test_under_unit_costs_rows_and_books_are_the_fitch_witnesss(alphabet, rule):
    """cost[x][y] = 1 off the diagonal: a per-pattern minimum is the Fitch length of the pattern, so one sweep books the same trees
    under the same lengths with the same rows, draws included"""
    n, P, B, radius = 9, 50, 8, 3
    codes, weights = tw.alignment(n, P, alphabet, 41)
    back = trees.random_topology(n, np.random.default_rng(3))
    samples = boot_samples(weights, B, 7)
    S = STATES[alphabet]
    unit = np.ones((S, S), dtype=np.uint32) - np.eye(S, dtype=np.uint32)
    a = make(codes, weights, alphabet, unit, 19, samples)
    b = make_fitch(codes, weights, alphabet, 19, samples)
    for w in (a, b):
        w.set_tree(back)
    assert a.length(back) == b.length(back) and (a.pattern_lengths(back) == b.pattern_lengths(back)).all()
    if rule == "cut":
        a.cutoff = b.cutoff = -float(a.length(back))
    assert a.tbr_sweep(radius) == b.tbr_sweep(radius)
    assert _state(a) == _state(b) and len(a.treels_logl) > 0 and a.ufb_draws > 0
    assert {t: list(x) for t, x in a.topologies.items()} == {t: list(x) for t, x in b.topologies.items()}
    for (where, ln, row) in a.rows:
        assert (row == b.pattern_lengths(trees.apply_tbr(back, tw.node_order(back, n)[where[0]],
                                                         *_pair(back, n, where, radius)))).all() and int(row @ weights) == ln


def _pair(back, n, where, radius):
    v, i, j = where
    F, G = tw.lists(back, n, tw.node_order(back, n)[v], radius)
    return ([tw.NONE] + [r for r, _ in F])[i], ([tw.NONE] + [r for r, _ in G])[j]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_gpu_cases_exercise_the_update_rule(case):
    codes, weights, cost, back, samples, radius, max_moves, w, cutoff = setup(case)
    plain = make(codes, weights, case["alphabet"], cost, 1, None)
    plain.set_tree(back)
    want = run(case, plain, radius, max_moves)
    got = run(case, w, radius, max_moves)
    assert got == want and w.back == plain.back and w.moves == plain.moves      # the bookkeeping does not steer the sweep or the climb
    sweeps = 1 if case["kind"] == "sweep" else got[1] + (1 if got[1] < max_moves else 0)
    assert plain.calls == [] and plain.draws == 0
    per_sweep, prev = 0, None
    for kind, (v, i, j), _t in w.calls:
        assert (kind == "cur") == (i == 0 and j == 0)
        if (v, i, j) == (0, 0, 0):
            per_sweep += 1
        elif prev is not None:
            pv, pi, pj = prev
            assert (v == pv and (i, j) > (pi, pj)) or (v == pv + 1 and (i, j) == (0, 0))
        prev = (v, i, j)
    assert per_sweep == sweeps
    if case["kind"] == "sweep":
        assert len(w.calls) == got[1]                                            # n_pairs: every entry once
    # every booked row sums to the length it was booked under
    assert len(w.rows) == len(w.treels_logl) > 0
    for _where, ln, row in w.rows:
        assert int(row @ weights) == ln
    assert shows_the_rule(case, w, got)
    assert w.ufb_draws > 0 or w.mulhits
    assert w.final_trees_booked_as_interior() >= 1
    if case["rule"] == "cut":
        acc, rej = w.candidate_calls()
        assert acc >= 1 and rej >= 1 and cutoff != 0.0
    if case["rule"] == "mulhits":
        assert w.largest_set >= 2
    if case["rule"] == "btrees":
        assert any(v != 0 for v in w.boot_tree_orig_logl)
    if case["kind"] == "climb":
        assert got[1] >= 2
    # the vectorised form books the same
    _c, _w, _m, _b, _s, _r, _mm, fb, _cut = setup(case, cls=FormB)
    assert run(case, fb, radius, max_moves) == got
    assert _state(fb) == _state(w) and fb.moves == w.moves
    assert all(a[:2] == b[:2] and (a[2] == b[2]).all() for a, b in zip(fb.rows, w.rows))


def test_the_large_shape_draws_and_books_interior_entries():
    """the witness's side of the one GPU shape above a single tile per row (FormB alone: form (a) would take minutes there)"""
    codes, weights, _cost, back, _samples, radius, _mm, w, _cut = setup(BIG, cls=FormB, sizes=(12, 260, 16, 2, 0))
    best, pairs = w.tbr_sweep(radius)
    assert pairs == len(w.calls) and w.ufb_draws > 0 and w.final_trees_booked_as_interior() >= 1
    assert codes.shape[1] == 260 and len(best) == 2 * 12 - 2
