"""CPU checks of the tracked TBR sweep's witness (tests/tbr_bb_witness.py): without samples its descent is TbrWitness.descent; the
identity the engine's mask rows rest on holds per pattern for every entry of every visit; and the inputs the GPU tests use
(tests/tbr_bb_cases.py) really exercise the tracker's update rule, so that no GPU test can pass on a run that booked nothing."""
import numpy as np
import pytest

import tbr_witness as tw
from mpboot_amd import trees
from tbr_bb_cases import CASES, DT, handover_steps, handover_witness, make, run, setup, shows_the_rule


@pytest.mark.parametrize("alphabet,n,P,radius", [("dna", 12, 120, 2), ("aa", 10, 60, 3), ("m32", 9, 40, 255)])
def test_without_samples_its_descent_is_the_plain_witnesses(alphabet, n, P, radius):
    codes, weights = tw.alignment(n, P, alphabet, 31 + n)
    back = trees.random_topology(n, np.random.default_rng(n))
    plain = tw.TbrWitness(codes, weights, DT[alphabet])
    want_back, want_len, want_moves = plain.descent(back, radius, 3)
    w = make(codes, weights, alphabet, 1, None)
    w.set_tree(back)
    assert w.length(back) == plain.length(back)
    best, pairs = w.tbr_sweep(radius)
    assert (best, pairs) == plain.sweep_best(back, radius) and w.back == back.tolist()
    assert w.optimize_tbr(radius, 3) == (want_len, len(want_moves))
    assert w.moves == want_moves and w.back == want_back.tolist() and len(want_moves) >= 1
    assert w.calls == [] and w.draws == 0


@pytest.mark.parametrize("alphabet", ["dna", "aa", "m32"])
def test_every_entrys_pattern_lengths_follow_from_two_masks(alphabet):
    """pattern_lengths(T_ij) == pattern_lengths(T) - M[0][0] + M[i][j] for every entry of every visit of a 12-taxon tree, M[i][j] =
    "R_q(F_i) and R_p(G_j) share no state" from TbrWitness.root_sets: each part's per-site length does not depend on its root"""
    n, P = 12, 70
    codes, weights = tw.alignment(n, P, alphabet, 77)
    back = trees.random_topology(n, np.random.default_rng(5))
    plain = tw.TbrWitness(codes, weights, DT[alphabet])
    w = make(codes, weights, alphabet, 1, None)
    base = w.pattern_lengths(back)
    views = plain.views(back)
    entries = 0
    for radius in (2, 255):
        for p in tw.node_order(back, n):
            q = int(back[p])
            F, G = tw.lists(back, n, p, radius)
            rf = [views[q][0]] + plain.root_sets(back, views, q, radius)
            rg = [views[p][0]] + plain.root_sets(back, views, p, radius)
            fr, gr = [tw.NONE] + [r for r, _ in F], [tw.NONE] + [r for r, _ in G]
            m00 = ((rf[0] & rg[0]) == 0).astype(np.int64)
            for i, f in enumerate(fr):
                for j, g in enumerate(gr):
                    mij = ((rf[i] & rg[j]) == 0).astype(np.int64)
                    assert (w.pattern_lengths(trees.apply_tbr(back, p, f, g)) == base - m00 + mij).all(), (radius, p, i, j)
                    entries += 1
    assert entries > 500


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_gpu_cases_exercise_the_update_rule(case):
    codes, weights, back, samples, radius, max_moves, w, cutoff = setup(case)
    plain = make(codes, weights, case["alphabet"], 1, None)
    plain.set_tree(back)
    want = run(case, plain, radius, max_moves)
    got = run(case, w, radius, max_moves)
    assert got == want and w.back == plain.back and w.moves == plain.moves      # the bookkeeping does not steer the sweep or the climb
    # booking order: per sweep the visits in order, each from [0][0], row-major; one call per entry
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


def test_the_hand_over_books_in_every_climb():
    """the witness's side of the GPU hand-over test: SPR, then TBR, then NNI tracked climbs on one tracker; each of them books"""
    _fx, _samples, starts, w = handover_witness()
    out, sizes = handover_steps(w, starts)
    assert 0 < sizes[0] < sizes[1] < sizes[2]
    assert out[1][1] >= 1 and w.ufb_draws > 0
