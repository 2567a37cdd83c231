"""The tracked NNI climb (mpf_ufboot_optimize_nni) under -storetrees, -mulhits -topboot N and -distinct_iter_top_boot k, and on a
sample-sharded tracker -- option "nni_tracked_rules" -- against the witness in tests/nni_bb_rules_witness.py.  Everything is
compared exactly, behind every climb of a case: treels_logl, boot_logl, boot_counts, boot_trees, the per-sample sets / top lists /
iterations / thresholds, the duplicate counter, the draw count and the 64-bit state of the tie stream, the tree, the swaps and the
number of trees handed over; the stored topologies at the end.  The cases are those of tests/nni_bb_rules_cases.py, which
tests/test_nni_bb_rules_witness.py shows to reach what each of them is there for.

Sharded: two engines of this process stand in for two ranks, each climbing in a thread of its own; their exchange call-backs meet
at a barrier and hand both the two parts in rank order."""
import ctypes as C
import threading

import numpy as np
import pytest

from helpers import same_topology
from nni_bb_rules_cases import FITCH, SEQUENCE, SHARDED, WEIGHTED, climbed, cost_matrix, drive, fixture, samples_of, sequence_inputs, sequence_witness
from nni_bb_rules_witness import shard_ids
from oracle.search_slow import LONG_MAX

pytestmark = pytest.mark.gpu


def _engine(case, rules=1):
    from mpboot_amd import engine
    fx = fixture(case)
    cost = cost_matrix(case)
    e = engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
    if cost is not None:
        e.set_option("nni_weighted", 1)
        e.set_option("nni_weighted_tracked", 1)
    elif case.get("tile", -1) != -1:
        e.set_option("nni_tile", case["tile"])
    e.set_option("nni_tracked_rules", rules)
    e.seed_ties(engine.TIE_RANDOM, 11)
    return e


def _set_rule(e, case):
    if case["rule"] in ("mulhits", "topboot"):
        e.ufboot_set_mulhits(True)
    if case["rule"] == "topboot":
        e.ufboot_set_topboot(case["arg"])
    if case["rule"] == "distinct":
        e.ufboot_set_distinct_iter(case["arg"])
    if case.get("store"):
        e.ufboot_set_store_trees(True)
    if not case.get("hclimb1_bb", True):
        e.ufboot_set_ratchet_booking(False)


def _books(e, case):
    """the engine's side of nni_bb_rules_cases.snapshot (without the climb's own fields)"""
    B = case["B"]
    logl, counts, trees = e.ufboot_state()
    listed = case["rule"] in ("topboot", "distinct")
    tops = [e.ufboot_sample_top(b) for b in range(B)] if listed else []
    return dict(treels_logl=e.ufboot_tree_logl().tolist(),
                boot_logl=[-LONG_MAX if v <= -LONG_MAX / 2 else v for v in logl.tolist()], boot_counts=counts.tolist(), boot_trees=trees.tolist(),
                boot_sets=[e.ufboot_sample_trees(b) for b in range(B)] if case["rule"] == "mulhits" else None,
                boot_top=[t for t, _thr in tops] if listed else None, boot_threshold=[thr for _t, thr in tops] if listed else None,
                boot_top_iter=[e.ufboot_sample_iters(b) for b in range(B)] if case["rule"] == "distinct" else None,
                duplicates=e.ufboot_duplicates(), ufb_draws=e.ufboot_counters()["tie_draws"], rng=e.tie_state(),
                back=e.get_tree().tolist(), log=[tuple(int(x) for x in m) for m in e.nni_moves()])


def _assert_books(got, want, case, where):
    for k, v in got.items():
        if v is None:
            continue
        if k == "boot_trees" and case["rule"] in ("mulhits", "topboot"):
            continue                                   # (boot_trees belongs to the default and the -distinct rule)
        assert v == want[k], (where, k)


def _assert_topologies(e, w, case, n):
    if case["rule"] == "mulhits":
        named = {t for s in w.boot_sets for t in s}
    elif case["rule"] == "topboot":
        named = {t for lst in w.boot_top for t, _r in lst}
    else:
        named = {t for t in w.boot_trees if t >= 0} | {t for lst in w.boot_top for t, _r in lst}
    assert named
    for t in sorted(named):
        assert same_topology(e.ufboot_tree(t), w.topologies[t], n), t


def _run(case):
    w, want_res, snaps = climbed(case["id"], False)
    n = fixture(case)["codes_np"].shape[0]
    e = _engine(case)
    e.ufboot_attach(samples_of(case))
    _set_rule(e, case)
    booked = [e.get_option("nni_booked")]

    def after(i):
        _assert_books(_books(e, case), snaps[i], case, i)
        booked.append(e.get_option("nni_booked"))
        assert booked[-1] - booked[0] == snaps[i]["calls"], i

    got = drive(e, case, after)
    assert got == want_res
    _assert_topologies(e, w, case, n)


@pytest.mark.parametrize("case", FITCH, ids=[c["id"] for c in FITCH])
def test_rules_on_the_fitch_engine(case):
    _run(case)


@pytest.mark.parametrize("case", WEIGHTED, ids=[c["id"] for c in WEIGHTED])
def test_rules_on_the_weighted_engine(case):
    _run(case)


class _Joint:
    """the exchange of two ranks that live in one process"""

    def __init__(self):
        from mpboot_amd import shard
        self.bar = threading.Barrier(2)
        self.part = [None, None]
        self.tag = [None, None]
        self.tags = []
        self.sizes = []
        self.keep = [None, None]
        self.cbs = [shard.EXCHANGE_FN(self._fn(r)) for r in range(2)]

    def _fn(self, rank):
        def fn(_arg, tag, local_ptr, n_local, all_ptr, n_all_ptr):
            try:
                self.part[rank] = (np.ctypeslib.as_array(C.cast(local_ptr, C.POINTER(C.c_uint32)), shape=(n_local, 3)).copy() if n_local
                                   else np.zeros((0, 3), dtype=np.uint32))
                self.tag[rank] = int(tag)
                self.bar.wait(timeout=120)
                if self.tag[0] != self.tag[1]:
                    return 2
                merged = np.ascontiguousarray(np.concatenate(self.part, axis=0))
                if rank == 0:
                    self.tags.append(int(tag))
                    self.sizes.append((len(self.part[0]), len(self.part[1])))
                self.keep[rank] = merged
                all_ptr[0] = merged.ctypes.data if len(merged) else None
                n_all_ptr[0] = len(merged)
                self.bar.wait(timeout=120)             # (nobody writes its next part before both have read this one)
                return 0
            except Exception:                          # a broken barrier included: the other rank failed
                return 1
        return fn


@pytest.mark.parametrize("case", SHARDED, ids=[c["id"] for c in SHARDED])
def test_two_ranks_equal_the_unsharded_engine_and_the_witness(case):
    w, want_res, snaps = climbed(case["id"], False)
    n = fixture(case)["codes_np"].shape[0]
    samples = samples_of(case)
    ids = shard_ids(case["B"], case["shard"])
    joint = _Joint()
    ranks = [_engine(case) for _ in range(2)]
    for r, e in enumerate(ranks):
        e.ufboot_attach(samples, shard=(r, 2), exchange=joint.cbs[r], sample_ids=ids[r])
        _set_rule(e, case)
    res, errs = [None, None], [None, None]
    books = [[], []]

    def work(r):
        try:
            res[r] = drive(ranks[r], case, lambda _i: books[r].append(_books(ranks[r], case)))
        except BaseException as exc:                   # noqa: BLE001 -- reported by the main thread
            errs[r] = exc
            joint.bar.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th)
    assert errs == [None, None], errs
    # both ranks == the witness, behind every climb
    for r in range(2):
        assert res[r] == want_res
        for i, b in enumerate(books[r]):
            _assert_books(b, snaps[i], case, (r, i))
        _assert_topologies(ranks[r], w, case, n)
    # == the unsharded engine
    one = _engine(case)
    one.ufboot_attach(samples)
    _set_rule(one, case)
    assert drive(one, case) == want_res
    assert _books(one, case) == books[0][-1] == books[1][-1]
    # one exchange per scoring step that books, under the NNI climb's own tags, and a closing one per climb; both ranks had events
    steps = [t for t in joint.tags if t != 0xFFFFFFFE]
    tracked = sum(1 for c in case["climbs"] if case.get("hclimb1_bb", True) or c["pert"] is None)
    assert joint.tags.count(0xFFFFFFFE) == tracked
    assert steps and all(0x40000000 <= t < 0x80000000 for t in steps)
    scoring = sum(1 for k, _s, _t in w.calls if k == "cur")
    # (the weighted step leaves early, before its product, when a cut-off turns the whole step away)
    assert len(steps) == scoring if "cost" not in case else 1 <= len(steps) <= scoring
    assert any(a > len(ids[0]) and b > len(ids[1]) for a, b in joint.sizes)        # (more than the current tree's own offers)


def test_spr_then_nni_then_spr_on_one_tracker_under_topboot():
    """what an SPR tracked climb left in the lists is what the NNI climb books into, and the other way round: the books behind
    each of the three calls are the witness's (nni_bb_rules_cases.sequence_witness, whose lists change in every call)"""
    from mpboot_amd import engine
    fx, samples, calls = sequence_inputs()
    n = fx["codes_np"].shape[0]
    w, want = sequence_witness()
    e = engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"])
    e.set_option("nni_tracked_rules", 1)
    e.seed_ties(engine.TIE_RANDOM, 11)
    e.ufboot_attach(samples)
    _set_rule(e, SEQUENCE)
    for k, (kind, back, radius) in enumerate(calls):
        e.set_tree(back)
        got = e.optimize_spr(1, radius) if kind == "spr" else tuple(e.ufboot_optimize_nni(1, True, 50))
        assert got == want[k][0], k
        books = _books(e, SEQUENCE)
        if kind == "spr":
            books.pop("log")                           # (the NNI swaps: not an SPR climb's)
        _assert_books(books, want[k][1], SEQUENCE, k)
    _assert_topologies(e, w, SEQUENCE, n)


def test_with_the_option_at_0_the_four_cases_are_refused_as_before():
    from mpboot_amd import engine, trees
    case = FITCH[0]
    fx = fixture(case)
    n = fx["codes_np"].shape[0]
    back = trees.random_topology(n, np.random.default_rng(1))
    samples = samples_of(case)

    def refusal(e):
        with pytest.raises(engine.MpfError) as ei:
            e.ufboot_optimize_nni(1)
        assert ei.value.code == -6
        assert len(e.ufboot_tree_logl()) == 0 and (e.get_tree() == back).all()
        return str(ei.value)

    setters = [(lambda x: x.ufboot_set_store_trees(True), "tracked NNI climb: -storetrees is not served"),
               (lambda x: (x.ufboot_set_mulhits(True), x.ufboot_set_topboot(3)), "tracked NNI climb: -mulhits -topboot is not served"),
               (lambda x: x.ufboot_set_distinct_iter(2), "tracked NNI climb: -distinct_iter_top_boot is not served")]
    for setter, msg in setters:
        x = _engine(case, rules=0)
        assert x.get_option("nni_tracked_rules") == 0
        x.set_tree(back)
        x.ufboot_attach(samples)
        setter(x)
        assert msg in refusal(x)
    joint = _Joint()
    sh = _engine(case, rules=0)
    sh.set_tree(back)
    sh.ufboot_attach(samples, shard=(0, 2), exchange=joint.cbs[0])
    assert "tracked NNI climb: not served with a sample-sharded tracker" in refusal(sh)
    assert joint.tags == []
    # the plain entry refuses a tracker whatever the option says
    p = _engine(case, rules=1)
    p.set_tree(back)
    p.ufboot_attach(samples)
    with pytest.raises(engine.MpfError) as ei:
        p.optimize_nni(1)
    assert ei.value.code == -6
    assert engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"]).get_option("nni_tracked_rules") == 0
