"""The witness of the tracked weighted NNI climb (tests/nni_snk_bb_witness.py) against what it is built from, and the committed
cases (tests/nni_snk_bb_cases.py) against what they are there for.  No GPU."""
import numpy as np
import pytest

from helpers import load_fixture
from nni_bb_cases import boot_samples
from nni_bb_witness import NniBbWitness
from nni_snk_bb_cases import CASES, climbed, setup, start_tree
from nni_snk_bb_witness import make
from nni_snk_witness import SnkNniWitness

IDS = [c["id"] for c in CASES]


@pytest.mark.parametrize("cid", IDS)
def test_every_booked_row_sums_to_the_length_it_was_booked_with(cid):
    (_fx, _cost, _n, root, _back, _samples, w, _cut), _want = climbed(cid)
    assert len(w.rows) == len(w.calls) > 0
    for kind, edge, length, row, bk in w.rows:
        assert int((row * w.w).sum()) == length
        if kind == "cur":
            assert edge is None and length == w.scorer.length(bk, root)
        else:
            assert length == w.scorer.edge_length(bk, *edge)


class _RecordingFitch(NniBbWitness):
    """NniBbWitness that keeps the row every call books"""

    def book(self, length, kind, step):
        self.booked_rows = getattr(self, "booked_rows", [])
        self.booked_rows.append(self.pattern_lengths(self.back).copy())
        NniBbWitness.book(self, length, kind, step)


@pytest.mark.parametrize("name,rule", [("dna_clean", None), ("dna_ambig", "mulhits"), ("aa", None), ("dna_dups", None)])
def test_unit_costs_are_the_fitch_witness(name, rule):
    """cost 1 - I: every row, current and candidate, is the Fitch row of that tree, and the complete books after a climb capped at
    one step are NniBbWitness(keep_all=True)'s (one step: the two rollback rules do not come into it)"""
    fx = load_fixture(name)
    S = fx["S"]
    samples = boot_samples(len(fx["weights"]), 8, 5, fx["weights"])
    back = start_tree(fx, 2)
    f = _RecordingFitch(fx["codes_np"], fx["weights_np"], fx["datatype"], np.ones(len(fx["weights"]), dtype=bool), 7, samples)
    w = make(fx, 1 - np.eye(S, dtype=np.int64), 7, samples)
    for x in (f, w):
        x.set_tree(back)
        x.mulhits = rule == "mulhits"
    assert w.optimize_nni(True, 1) == f.optimize_nni(True, 1)
    assert len(w.rows) == len(f.booked_rows) > 1
    for (_k, _e, _l, row, _bk), frow in zip(w.rows, f.booked_rows):
        assert (row == frow).all()
    assert w.treels_logl == f.treels_logl and len(w.treels_logl) == len(w.calls)
    assert (w.boot_logl, w.boot_counts, w.boot_trees) == (f.boot_logl, f.boot_counts, f.boot_trees)
    assert w.boot_sets == f.boot_sets
    assert w.topologies == f.topologies
    assert (w.ufb_draws, int(w.rng.state)) == (f.ufb_draws, int(f.rng.state))
    assert [(k, t) for k, _s, t in w.calls] == [(k, t) for k, _s, t in f.calls]
    assert list(w.back) == list(f.back) and w.log == f.log


@pytest.mark.parametrize("cid", IDS)
def test_without_samples_it_is_the_plain_weighted_witness(cid):
    case = next(c for c in CASES if c["id"] == cid)
    fx, cost, n, root, back, _samples, _w, _cut = setup(case)
    steps = case.get("steps", 50)
    w = make(fx, cost, case["tie"], None, root)
    w.set_tree(back)
    p = SnkNniWitness(back, n, w.scorer, root_taxon=root)
    assert w.optimize_nni(case["speednni"], steps) == p.optimize(case["speednni"], steps)
    assert w.log == p.log and list(w.back) == p.back.tolist()
    assert (w.kept_worse, w.most_applied) == (p.kept_worse, p.most_applied)
    assert w.calls == [] and w.draws == 0


@pytest.mark.parametrize("cid", IDS)
def test_every_case_exercises_the_update_rule(cid):
    case = next(c for c in CASES if c["id"] == cid)
    (_fx, _cost, _n, _root, _back, _samples, w, cut), want = climbed(cid)
    assert w.ufb_draws > 0 or w.mulhits
    assert w.final_trees_booked_as_candidates() >= 1
    if cut:
        acc, rej = w.candidate_calls()
        assert acc > 0 and rej > 0
    # no rollback steps: every step that ran booked its current tree
    assert sum(1 for k, _s, _t in w.calls if k == "cur") == min(want[2], case.get("steps", 50))


def test_some_case_keeps_a_worse_step_and_books_the_tree_behind_it():
    hit = 0
    for cid in IDS:
        (_fx, _cost, _n, root, _back, _samples, w, _cut), _want = climbed(cid)
        if not w.kept_worse:
            continue
        # the current tree of some step is LONGER than the best candidate the step before promised, and it is booked under that length
        cur = [(i, r) for i, r in enumerate(w.rows) if r[0] == "cur"]
        for (i0, _r0), (i1, r1) in zip(cur, cur[1:]):
            best = min(r[2] for r in w.rows[i0 + 1:i1])
            if r1[2] > best:
                hit += 1
                assert w.calls[i1][0] == "cur" and r1[2] == w.scorer.length(r1[4], root)
    assert hit > 0


def test_some_asym_candidate_row_depends_on_its_edge():
    """what makes the orientation matter: under a matrix that is not symmetric a booked candidate's row (at its branch, node2's
    side the parent) is not that tree's root-leaf row"""
    differ = 0
    for case in CASES:
        if case["cost"] != "asym":
            continue
        (_fx, _cost, _n, root, _back, _samples, w, _cut), _want = climbed(case["id"])
        differ += sum(1 for kind, _e, _l, row, bk in w.rows[:200] if kind == "cand" and (row != w.scorer.root_row(bk, root)).any())
    assert differ > 0
