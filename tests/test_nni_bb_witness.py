"""CPU checks of the tracked NNI climb's witness (tests/nni_bb_witness.py): without samples it is NniWitness; with samples it
calls saveCurrentTree 1 + 2 * branches times per scoring step, in booking order; and the inputs the GPU tests use
(tests/nni_bb_cases.py) really exercise the tracker's update rule, so that no GPU test can pass on a run that booked nothing."""
import numpy as np
import pytest

from helpers import FIXTURES, load_fixture
from nni_bb_cases import CASES, boot_samples, setup, start_tree
from nni_bb_witness import make
from nni_witness import NniWitness
from oracle import pyoracle as po


@pytest.mark.parametrize("name,start,speednni,root", [("dna_clean", ("random", 0), True, 1), ("dna_dups", ("random", 1), True, 1),
                                                      ("bin", ("random", 2), False, "n"), ("aa", ("stepwise", 1), True, 1),
                                                      ("morph32", ("random", 4), False, 1)])
def test_without_samples_it_is_the_plain_witness(name, start, speednni, root):
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    root = n if root == "n" else 1
    back = start_tree(fx, start)
    o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"])
    plain = NniWitness(back, n, lambda b: o.score_tree(b), root_taxon=root)
    want = plain.optimize(speednni=speednni)
    w = make(fx, 1, None, root)
    w.set_tree(back)
    assert w.optimize_nni(speednni=speednni) == want
    assert w.back == plain.back.tolist()
    assert w.log == plain.log and w.rollbacks == plain.rollbacks
    assert w.calls == [] and w.draws == 0


@pytest.mark.parametrize("keep_all", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_from_scratch_lengths_are_the_pinned_oracles(name, keep_all):
    """every alphabet the GPU cases use (SlowSearch itself knows DNA and protein), with and without the dropped patterns"""
    fx = load_fixture(name)
    o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], keep_all=keep_all)
    w = make(fx, 1, None, 1, keep_all=keep_all)
    for t in fx["trees"][:4]:
        assert w.length(t["back"]) == o.score_tree(np.array(t["back"], dtype=np.int32))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_gpu_cases_exercise_the_update_rule(case):
    fx, n, root, back, samples, w, cutoff = setup(case)
    plain = make(fx, 1, None, root, case.get("keep_all", False))
    plain.set_tree(back)
    want = plain.optimize_nni(speednni=case["speednni"])
    got = w.optimize_nni(speednni=case["speednni"])
    assert got == want and w.back == plain.back and w.log == plain.log          # the bookkeeping does not steer the climb
    # booking order and number of calls: per step that is not a rollback step the current tree, then two per evaluated branch
    steps = {}
    for kind, step, _t in w.calls:
        steps.setdefault(step, []).append(kind)
    for step, kinds in steps.items():
        assert kinds[0] == "cur" and all(k == "cand" for k in kinds[1:]) and len(kinds) % 2 == 1 and len(kinds) >= 3
    assert len(steps) == got[2] - w.rollbacks - (1 if got[2] > 50 else 0)
    if not case["speednni"]:
        assert all(len(k) == 1 + 2 * (n - 3) for k in steps.values())
    if case["id"].count("rollback"):
        assert w.rollbacks >= 1
    # the rule is exercised
    if case.get("rule") == "mulhits":
        assert w.largest_set >= 2 and any(w.kind_of.get(t) == "cand" for s in w.boot_sets for t in s)
    else:
        assert w.ufb_draws > 0
        assert w.final_trees_booked_as_candidates() >= 1
    if case.get("cut"):
        acc, rej = w.candidate_calls()
        assert acc >= 1 and rej >= 1
    if case.get("btrees"):
        assert any(v != 0 for v in w.boot_tree_orig_logl)


def test_sequence_books_in_every_climb():
    """the witness's side of the GPU sequence test: short normal climb / ratchet climb under a cut-off / normal climb, then an
    SPR climb.  Every climb books; the ratchet one under its trees' own lengths on the original alignment, with candidates on
    both sides of the cut-off and one that a sample takes"""
    from mpboot_amd import engine
    fx = load_fixture("dna_clean")
    w0 = fx["weights_np"]
    samples = boot_samples(len(fx["weights"]), 8, 21, fx["weights"])
    w = make(fx, 31, samples)
    starts = [start_tree(fx, ("random", s)) for s in (5, 6, 7)]
    w.set_tree(starts[0])
    w.optimize_nni(True, 2)
    n1, d1 = len(w.treels_logl), w.ufb_draws
    assert n1 > 0 and d1 > 0
    w.cutoff = float(np.sort(np.array(w.treels_logl))[int(n1 * 0.97)])
    pert, _st = engine.iq_perturb_weights(w0, fx["informative"], 50, 1, 12345)
    w.set_weights(pert)
    assert w.ratchet
    w.set_tree(starts[1])
    first = w.length(w.back)
    calls0 = len(w.calls)
    w.optimize_nni(False)
    n2 = len(w.treels_logl)
    assert n2 > n1
    ref = make(fx, 1, None)
    # lengths are those on the ORIGINAL weights: the start tree fails the cut-off by it, and the last step's current tree -- the
    # final tree -- is booked under it
    assert w.calls[calls0] == ("cur", 1, None) and -ref.length(starts[1]) <= w.cutoff - 1e-4
    last = [t for k, _s, t in w.calls[calls0:] if k == "cur"][-1]
    assert last is not None and -w.treels_logl[last] == ref.length(w.back) != w.length(w.back) and first != ref.length(starts[1])
    mine = [(k, t) for k, _s, t in w.calls[calls0:] if k == "cand"]
    assert any(t is not None for _k, t in mine) and any(t is None for _k, t in mine)
    assert any(m and k == "cand" for m, (k, _s, _t) in zip(w.took[calls0:], w.calls[calls0:]))
    w.set_weights(w0)
    w.set_tree(starts[2])
    w.optimize_nni()
    n3 = len(w.treels_logl)
    assert n3 > n2
    w.optimize(1, 3)
    assert len(w.treels_logl) > n3
