"""CPU checks of the witness of the tracked NNI climb under the optional update rules (tests/nni_bb_rules_witness.py):

  * its restatement of saveCurrentTree agrees with oracle/search_slow.py's on the part they share -- both are fed the same
    sequence of (tree, row of per-pattern lengths, length) offers and every book, count and draw is compared;
  * two shards whose offers are merged give the unsharded books;
  * every case the GPU test runs (tests/nni_bb_rules_cases.py) reaches, on the witness alone, what makes it a test.

-storetrees, as the reference has it (iqtree.cpp:3302-3351, and Engine::ufb_book_tree): a topology met before is counted and
goes on only with a better length than the recorded one -- then WITHOUT the cut-off test; a new topology that fails the cut-off is
not stored.  "Stored although it fails the cut-off" is therefore a known topology that comes back with a better length that fails
the cut-off in force.  Under NNI a tree's booked length is its own, a function of the topology on the Fitch engine and on a
symmetric matrix at one root; it differs between two visits only where the row's edge matters (an asymmetric matrix: a candidate
is scored at its own branch).  The assertion is made where that happens, and the other -storetrees cases assert duplicates and
new topologies turned away by the cut-off.
"""
import numpy as np
import pytest

from nni_bb_rules_cases import (ALL, FITCH, SHARDED, WEIGHTED, WitnessDriver, by_id, climbed, drive, fixture, new_witness, samples_of, sequence_witness,
                                snapshot)
from nni_bb_rules_witness import set_rule, shard_ids
from oracle.search_slow import SlowSearch

IDS = [c["id"] for c in ALL]


def _offers_of(case_id):
    """every saveCurrentTree call of the case's climbs as the witness saw it: (back, row, length, ratchet, cut-off, iteration)"""
    case = by_id(case_id)
    w = new_witness(case)
    rec = []
    inner = w.save_current_tree

    def spy(cur_logl):
        if w.bb_on:
            rec.append((list(w.back), np.array(w.pattern_pars), cur_logl, w.ratchet, w.cutoff, w.cur_it, np.array(w.w)))
        inner(cur_logl)

    w.save_current_tree = spy
    drive(WitnessDriver(w), case)
    return w, rec


class _Replay(SlowSearch):
    """SlowSearch fed a recorded offer: the row comes from the record, not from a scorer"""

    def pattern_lengths(self, back):
        return self._row


@pytest.mark.parametrize("case_id", [c["id"] for c in FITCH + WEIGHTED])
def test_the_restatement_agrees_with_search_slows_tracker(case_id):
    case = by_id(case_id)
    fx = fixture(case)
    w, rec = _offers_of(case_id)
    assert len(rec) > 20
    ones = np.ones(len(fx["weights"]), dtype=bool)
    s = _Replay(fx["codes_np"], fx["weights_np"], fx["datatype"], w.inf if "cost" not in case else ones, 11, samples_of(case))
    set_rule(s, case["rule"], case.get("arg", 0), case.get("store", False))
    for back, row, cur_logl, ratchet, cutoff, it, wgt in rec:
        s.back, s._row, s.pattern_pars = back, row, row
        s.ratchet, s.cutoff, s.cur_it = ratchet, cutoff, it
        s.save_current_tree(cur_logl)
    for k in ("treels_logl", "boot_logl", "boot_counts", "boot_trees", "boot_top", "boot_top_iter", "boot_threshold", "duplicates", "ufb_draws",
              "boot_tree_orig_logl"):
        assert getattr(s, k) == getattr(w, k), k
    assert [sorted(x) for x in s.boot_sets] == [sorted(x) for x in w.boot_sets]
    assert s.treels == w.treels and int(s.rng.state) == int(w.rng.state)
    assert s.rebooked == w.dup_improved


@pytest.mark.parametrize("case_id", [c["id"] for c in SHARDED])
def test_two_shards_are_the_unsharded_books(case_id):
    case = by_id(case_id)
    one, res1, snaps1 = climbed(case_id, False)
    two, res2, snaps2 = climbed(case_id, True)
    assert res1 == res2 and snaps1 == snaps2
    ids = shard_ids(case["B"], case["shard"])
    assert sorted(ids[0] + ids[1]) == list(range(case["B"])) and not set(ids[0]) & set(ids[1])
    # a step in which offers of BOTH shards changed some sample's books
    assert any(v == {0, 1} for v in two.shard_steps.values())


@pytest.mark.parametrize("case_id", IDS)
def test_gpu_cases_reach_what_they_are_there_for(case_id):
    case = by_id(case_id)
    w, res, snaps = climbed(case_id, False)
    assert len(res) == len(case["climbs"]) and all(r[2] >= 2 for r in res)
    assert len(w.calls) > 0 and len(w.treels_logl) > 0
    booked = [s["treels_logl"] for s in snaps]
    if case.get("hclimb1_bb", True):
        assert all(len(a) < len(b) for a, b in zip(booked, booked[1:])) or case.get("store")       # every climb books
    else:
        assert booked[0] == booked[1] and len(booked[2]) > len(booked[1])                          # the ratchet climb books nothing
    if case.get("store"):
        # duplicates, and (under a cut-off) new topologies the cut-off turned away although the product could not skip them
        assert w.duplicates >= 1
        if any(c["cut"] for c in case["climbs"]) and case.get("hclimb1_bb", True):
            assert w.new_failed_cut >= 1
    if case["rule"] == "topboot":
        N = case["arg"]
        assert any(len(t) == N for t in w.boot_top) and w.displaced >= 1
        assert all(len(t) <= N and [r for _t, r in t] == sorted((r for _t, r in t), reverse=True) for t in w.boot_top)
    if case["rule"] == "distinct":
        k = case["arg"]
        assert any(len(t) == k for t in w.boot_top) and w.ufb_draws >= 1
        if k > 1 or len({c["it"] for c in case["climbs"]}) < len(case["climbs"]):
            assert w.offers_rejected_same_iter >= 1
    if case["rule"] == "default":
        assert w.ufb_draws >= 1
    if case["rule"] == "mulhits":
        assert w.largest_set >= 2


def test_some_store_case_books_past_the_cut_off_and_topboot_draws_nothing_itself():
    """across the -storetrees cases at least one known topology is booked again, with a better length, past the cut-off in force.
    The -mulhits rules draw nothing (iqtree.cpp:3498-3583 has no random_double) and an NNI climb has no draws of its own, so the
    tie draws of a -topboot run are those of the SPR climbs around it: test_the_sequence_changes_the_lists_in_every_call"""
    ws = [climbed(c["id"], False)[0] for c in ALL if c.get("store")]
    assert sum(w.dup_improved for w in ws) >= 1
    assert sum(w.dup_improved_past_cut for w in ws) >= 1
    assert all(climbed(c["id"], False)[0].ufb_draws == 0 for c in ALL if c["rule"] in ("topboot", "mulhits"))


def test_snapshots_are_plain_data():
    w, _res, snaps = climbed(IDS[0], False)
    assert snapshot(w) == snaps[-1]


def test_the_sequence_changes_the_lists_in_every_call():
    """SPR, NNI, SPR on one tracker under -topboot 3: every call books, changes some sample's list and displaces entries of full
    lists; the shared stream moves in the SPR climbs (their own tie rule)"""
    w, out = sequence_witness()
    snaps = [s for _r, s in out]
    assert len(snaps[0]["treels_logl"]) < len(snaps[1]["treels_logl"]) < len(snaps[2]["treels_logl"])
    assert snaps[0]["boot_top"] != snaps[1]["boot_top"] and snaps[1]["boot_top"] != snaps[2]["boot_top"]
    assert all(len(t) == 3 for t in snaps[0]["boot_top"]) and w.displaced >= 1
    assert snaps[0]["rng"] != snaps[2]["rng"] and w.draws > 0 and w.ufb_draws == 0
    assert snaps[1]["rng"] == snaps[0]["rng"]                      # (the NNI climb in between draws nothing under this rule)
