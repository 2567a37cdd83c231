"""The far end of a device-planned sweep step (option sweep_ends; Engine::set_tree, schedule_views_dev, launch_refresh and
sweep_scan_dev in mpboot_amd/csrc/engine.cpp, k_cntsum_slots and k_newview_self in kernels.hip, mpboot_amd/host/tree_links.hpp).

sweep_ends = 2 (the default): the refresh's mutation counts reach the host when their fold ends (a flag raised by the fold's last
workgroup) and the host makes the subtree scores and the scan parts' base lengths while the scan runs.  0 is the step of before.
(Bit 1, the early upload of the topology array from mpf_set_tree, was measured and not kept: the cases about handing trees over
stay, they hold for the one walk that now checks the links in mpf_set_tree and lays the array out for the refresh.)  The settings
are compared with each other and with the oracle's sweep (every prune node's candidates from rearrange, as
tests/test_gpu_pitch.py collects them).  Integer work: every comparison is exact.

Shapes: 8 taxa x 33 patterns (the smallest tree the device-planned route takes, one word plus one site), 9 x 2 049 (past a 64-word
scan tile), 40 x 300."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(8, 33), (9, 2049), (40, 300)]
SETTINGS = (2, 0)


@pytest.fixture(scope="module")
def mods():
    from mpboot_amd import engine, synth, trees
    from oracle import pyoracle as po
    return engine, po, synth, trees


_cases = {}


def _oracle_sweep(o, back, radius, n):
    """(insertion tests, best length) of a whole sweep of the oracle's, and the tree's length"""
    cur = o.score_tree(back)
    tests, lo = 0, None
    for r in o.nodep()[1:2 * n - 1]:
        o.set_best(cur)
        o.trace(True)
        o.rearrange(int(r), 1, radius)
        tq, tm = o.get_trace()
        keep = tq >= 0
        tests += int(keep.sum())
        if keep.any():
            m = int(tm[keep].min())
            lo = m if lo is None else min(lo, m)
    assert (o.get_tree() == back).all()
    return (tests, lo), cur


def _case(mods, n, P):
    """alignment, two topologies and the oracle's answers for them, made once per shape and left alone"""
    engine, po, synth, trees = mods
    if (n, P) not in _cases:
        # (synth_alignment hands out distinct patterns: 8 and 9 taxa at 6 % divergence have few -- a block of them is repeated)
        base = P if n >= 40 else 33
        letters, _ = synth.synth_alignment(n, base, "DNA", 0.08, seed=10 * n + 1)
        codes = np.tile(synth.letters_to_codes(letters, "DNA"), (1, (P + base - 1) // base))[:, :P]
        codes = np.ascontiguousarray(codes)
        rng = np.random.default_rng(n + P)
        A = trees.random_topology(n, rng)
        B = trees.random_topology(n, rng)
        while (B == A).all():
            B = trees.random_topology(n, rng)
        o = po.Oracle(codes, keep_all=True)
        o.seed_ties(po.TIE_RANDOM, 1)
        rad = min(6, n - 3)
        want = {"A": _oracle_sweep(o, A, rad, n), "B": _oracle_sweep(o, B, rad, n)}
        w = np.random.default_rng(3).integers(0, 3, size=P).astype(np.int32)
        w[0] = 1
        ow = po.Oracle(codes, weights=w, keep_all=True)
        ow.seed_ties(po.TIE_RANDOM, 1)
        want["Aw"] = _oracle_sweep(ow, A, rad, n)
        oc = po.Oracle(codes, keep_all=True)
        oc.seed_ties(po.TIE_RANDOM, 7)
        oc.score_tree(A)
        want["climb"] = (oc.optimize_spr(1, 6), oc.get_tree().tolist())
        _cases[(n, P)] = (codes, A, B, rad, w, want)
    return _cases[(n, P)]


def _engine(mods, codes, ends, **opts):
    engine = mods[0]
    e = engine.FitchEngine(codes, keep_all=True)
    e.set_option("sweep_ends", ends)
    for k, v in opts.items():
        e.set_option(k, v)
    assert e.get_option("sweep_ends") == ends
    return e


def _sweep(e, rad):
    k, best = e.sweep_scan(1, rad)
    return int(k), int(best)


@pytest.mark.parametrize("n,P", SHAPES)
def test_one_sweep_every_setting(mods, n, P):
    """set_tree(A), sweep_scan: the oracle's (tests, best) under every setting, and the sweep says which halves it used"""
    codes, A, B, rad, w, want = _case(mods, n, P)
    for ends in SETTINGS:
        e = _engine(mods, codes, ends)
        e.set_tree(A)
        assert _sweep(e, rad) == want["A"][0], ends
        assert e.get_option("sweep_ends_active") == ends
        assert e.get_option("refresh_self_sched_active") == 1
        assert e.score_tree() == want["A"][1]
        e.close()


@pytest.mark.parametrize("n,P", SHAPES)
def test_two_trees_no_sweep_between(mods, n, P):
    """set_tree(A), set_tree(B), sweep_scan: B's sweep; ten times, A and B taking turns (a layout must not outlive its tree)"""
    codes, A, B, rad, w, want = _case(mods, n, P)
    for ends in SETTINGS:
        e = _engine(mods, codes, ends, plan_cache=0)
        for i in range(10):
            first, second = (A, B) if i % 2 == 0 else (B, A)
            e.set_tree(first)
            e.set_tree(second)
            assert _sweep(e, rad) == want["B" if i % 2 == 0 else "A"][0], (ends, i)
            assert e.get_option("sweep_ends_active") == ends
        e.close()


@pytest.mark.parametrize("n,P", SHAPES)
@pytest.mark.parametrize("cache", [7, 0])
def test_same_tree_twice(mods, n, P, cache):
    """set_tree(A) twice, then the sweep: the same result, one copy of the topology array; the swept tree handed over once more:
    with the plan cache on the array stays where it is, with it off it goes up again"""
    codes, A, B, rad, w, want = _case(mods, n, P)
    for ends in SETTINGS:
        e = _engine(mods, codes, ends, plan_cache=cache)
        e.set_tree(A)
        e.set_tree(A)
        assert e.get_option("kids_uploads") == 0     # (mpf_set_tree sends nothing)
        assert _sweep(e, rad) == want["A"][0], ends
        assert e.get_option("kids_uploads") == 1
        e.set_tree(A)
        assert _sweep(e, rad) == want["A"][0], ends
        assert e.get_option("kids_uploads") == (1 if cache == 7 else 2)
        e.close()


@pytest.mark.parametrize("n,P", SHAPES)
@pytest.mark.parametrize("between", ["score_tree", "sweep_costs", "set_weights", "optimize_spr"])
def test_other_call_between_set_tree_and_sweep(mods, n, P, between):
    """another route behind set_tree stages its own topology array: its value is right, and so is the sweep after it"""
    engine, po, synth, trees = mods
    codes, A, B, rad, w, want = _case(mods, n, P)
    for ends in SETTINGS:
        e = _engine(mods, codes, ends)
        e.seed_ties(engine.TIE_RANDOM, 7)
        if between != "optimize_spr":                # (a sweep renumbers the node order a climb visits: the oracle's climb starts fresh)
            e.set_tree(B)
            assert _sweep(e, rad) == want["B"][0]
        e.set_tree(A)
        if between == "score_tree":
            assert e.score_tree() == want["A"][1]
            assert _sweep(e, rad) == want["A"][0], ends
        elif between == "sweep_costs":
            k, mp, _ = e.sweep_costs(1, rad)
            assert (int(k), int(mp.min())) == want["A"][0]
            assert _sweep(e, rad) == want["A"][0], ends
        elif between == "set_weights":
            e.set_weights(w)
            assert _sweep(e, rad) == want["Aw"][0], ends
            assert e.score_tree() == want["Aw"][1]
        else:
            assert e.optimize_spr(1, 6) == want["climb"][0]
            assert e.get_tree().tolist() == want["climb"][1]
            e.set_tree(A)
            assert _sweep(e, rad) == want["A"][0], ends
        e.close()


@pytest.mark.parametrize("n,P", SHAPES)
def test_scores_and_counts_whole_after_the_sweep(mods, n, P):
    """behind a sweep whose counts went ahead: score_tree() and pattern_scores() as behind the step of before"""
    codes, A, B, rad, w, want = _case(mods, n, P)
    got = {}
    for ends in SETTINGS:
        e = _engine(mods, codes, ends)
        e.set_tree(A)
        sw = _sweep(e, rad)
        s = e.score_tree()
        ptn, tot = e.pattern_scores()
        k, mp, off = e.sweep_costs(1, rad)
        got[ends] = (sw, s, int(tot), ptn.tolist(), int(k), mp.tolist(), off.tolist())
        e.close()
    for ends in SETTINGS:
        assert got[ends] == got[0], ends
    assert got[0][0] == want["A"][0] and got[0][1] == want["A"][1] and got[0][2] == want["A"][1]


@pytest.mark.parametrize("n,P", SHAPES)
def test_inconsistent_link_is_rejected(mods, n, P):
    """one link that is not answered: MPF_E_INVALID and the same message under every setting, nothing sent, and the tree the engine
    had is swept as before"""
    engine, po, synth, trees = mods
    codes, A, B, rad, w, want = _case(mods, n, P)
    bad = B.copy()
    r = 3 * (n + 2) + 1
    bad[r] = 3 * (n + 1) if int(B[r]) != 3 * (n + 1) else 3 * (n + 1) + 1
    msgs = set()
    for ends in SETTINGS:
        e = _engine(mods, codes, ends)
        e.set_tree(A)
        assert _sweep(e, rad) == want["A"][0]
        ups = e.get_option("kids_uploads")
        with pytest.raises(engine.MpfError) as err:
            e.set_tree(bad)
        assert err.value.code == -2                  # MPF_E_INVALID
        msgs.add(str(err.value))
        assert e.get_option("kids_uploads") == ups
        assert (e.get_tree() == A).all()
        assert _sweep(e, rad) == want["A"][0], ends
        assert e.score_tree() == want["A"][1]
        e.set_tree(B)
        assert _sweep(e, rad) == want["B"][0], ends
        e.close()
    assert len(msgs) == 1 and "inconsistent back links" in msgs.pop()


@pytest.mark.parametrize("kind", ["protein", "weighted"])
def test_engines_the_route_does_not_serve(mods, kind):
    """12 taxa x 40 patterns, protein and under a cost matrix: neither end is the device-planned step's; same results with the
    switch at 2 and at 0"""
    engine, po, synth, trees = mods
    n, P = 12, 40
    alpha = "AA" if kind == "protein" else "DNA"
    letters, _ = synth.synth_alignment(n, P, alpha, 0.08, seed=21)
    codes = synth.letters_to_codes(letters, alpha)
    back = trees.random_topology(n, np.random.default_rng(22))
    got = {}
    for ends in (2, 0):
        if kind == "protein":
            e = engine.FitchEngine(codes, datatype=engine.AA)
        else:
            cost = (np.ones((4, 4), dtype=np.uint32) - np.eye(4, dtype=np.uint32)) * 2
            cost[0, 2] = cost[2, 0] = cost[1, 3] = cost[3, 1] = 1
            e = engine.FitchEngine(codes, cost=cost)
        e.set_option("sweep_ends", ends)
        e.set_tree(back)
        sw = _sweep(e, 6)
        active = e.get_option("sweep_ends_active")
        k, mp, _ = e.sweep_costs(1, 6)
        got[ends] = (sw, e.score_tree(), int(k), mp.tolist())
        assert sw == (int(k), int(mp.min()))
        if kind == "weighted":
            assert active == 0
        e.close()
        got[(ends, "active")] = active
    assert got[2] == got[0]
    assert got[(0, "active")] == 0
    assert got[(2, "active")] == 0
