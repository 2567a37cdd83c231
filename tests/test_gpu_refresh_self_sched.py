"""The from-scratch refresh that schedules itself (option refresh_self_sched; k_newview_self, k_kids_copy and k_cntsum_slots in
mpboot_amd/csrc/kernels.hip, Engine::schedule_views_dev / launch_refresh in engine.cpp).

With refresh_self_sched = 1 (the default) a complete tree that has no valid vector is refreshed without a schedule: every refresh
workgroup finds the dependency levels itself, in LDS, from the topology array; no k_sched launch stands in front.  The reference of
every comparison is the same engine with refresh_self_sched = 0, the route from before the option existed (k_sched, then
k_newview_wgq); score_tree(back) is also asked of the CPU oracle.  Integer work: every comparison is exact.

Shapes: 4 taxa (three inner records, the smallest tree the route admits), 5 (one inner level), 33 (levels narrower than one round
of a workgroup), 343 and 344 taxa (1 023 and 1 026 records: either side of one record per thread), rows of 32 and 96 words on
refresh tiles of 8 and 32 words.  Every tree the device scheduler takes (kSchedMaxSlots vectors) fits the route's LDS, so there
is no tree between the two bounds to send the other way."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SITES = {32: 1000, 96: 3000}                         # sites -> Wp = 32-site words, padded to a multiple of 32
BOOKS = ("view_launches", "newview_ops", "plan_launches", "scan_launches")


@pytest.fixture(scope="module")
def mods():
    from mpboot_amd import engine, synth, trees
    from oracle import pyoracle as po
    return engine, po, synth, trees


_data = {}


def _codes(mods, n, wp, alpha="DNA"):
    """the alignment of a shape, made once per module"""
    engine, po, synth, trees = mods
    if (n, wp, alpha) not in _data:
        # (synth_alignment hands out DISTINCT patterns and few taxa have few of them -- 4^4 = 256, 4^5 = 1024: wider rows repeat a block)
        base = 200 if n == 4 else min(SITES[wp], 1000) if n == 5 else SITES[wp]
        letters, _ = synth.synth_alignment(n, base, alpha, 0.08, seed=100 * n + wp)
        _data[(n, wp, alpha)] = np.tile(synth.letters_to_codes(letters, alpha), (1, SITES[wp] // base))
    return _data[(n, wp, alpha)]


def _engine(mods, codes, self_sched, tile=0, datatype=None, **opts):
    engine = mods[0]
    e = engine.FitchEngine(codes) if datatype is None else engine.FitchEngine(codes, datatype=datatype)
    e.set_option("refresh_self_sched", self_sched)
    if tile:
        e.set_option("views_tile", tile)
    for k, v in opts.items():
        e.set_option(k, v)
    assert e.get_option("refresh_self_sched") == self_sched
    return e


def _sweep(e, r):
    """everything a sweep of radius r reports: the timed call's (tests, best) and every candidate of the same sweep"""
    k, best = e.sweep_scan(1, r)
    n, mp, off = e.sweep_costs(1, r)
    return int(k), int(best), int(n), mp.tolist(), off.tolist()


def _everything(e, back):
    """the values the issue names, each from a tree just handed over"""
    res = []
    for r in (1, 3, 6):
        e.set_tree(back)
        res.append(_sweep(e, r))
        res.append(e.score_tree())
    res.append(e.score_tree(back))                   # from scratch, then the evaluate alone
    route = e.get_option("refresh_self_sched_active")
    levels = e.get_option("sched_levels")
    ptn, tot = e.pattern_scores()
    res.append((int(tot), ptn.tolist()))
    return res, route, levels


def _caterpillar(trees, n):
    back = trees.empty_back(n)
    v = n + 1
    for s, t in enumerate((1, 2, 3)):
        back[3 * v + s] = 3 * t
        back[3 * t] = 3 * v + s
    for t in range(4, n + 1):
        v += 1
        e = 3 * (t - 1)
        f = int(back[e])
        back[3 * v] = 3 * t
        back[3 * t] = 3 * v
        back[3 * v + 1] = e
        back[e] = 3 * v + 1
        back[3 * v + 2] = f
        back[f] = 3 * v + 2
    trees.validate(back, n)
    return back


def _balanced(trees, n):
    names = ["t%d" % i for i in range(n)]

    def sub(lo, hi):
        if hi - lo == 1:
            return names[lo]
        mid = (lo + hi) // 2
        return "(" + sub(lo, mid) + "," + sub(mid, hi) + ")"

    a, b = n // 3, 2 * n // 3
    return trees.newick_to_back("(" + sub(0, a) + "," + sub(a, b) + "," + sub(b, n) + ");", names)


@pytest.mark.parametrize("n,wp", [(4, 32), (5, 96), (33, 96), (343, 32), (344, 32)])
@pytest.mark.parametrize("tile", [8, 32])
def test_equals_the_scheduled_refresh(mods, n, wp, tile):
    """sweep_scan(1, r) for r = 1, 3, 6, sweep_costs(1, r), score_tree() and pattern_scores() of a tree just handed over, with the
    switch on and off; score_tree(back) against the oracle; the level count against k_sched's"""
    engine, po, synth, trees = mods
    codes = _codes(mods, n, wp)
    back = trees.random_topology(n, np.random.default_rng(n + wp))
    got = {}
    for on in (0, 1):
        e = _engine(mods, codes, on, tile, plan_cache=0)
        assert e.Wp == wp
        got[on] = _everything(e, back)
        e.close()
    assert got[1][1] == 1 and got[0][1] == 0         # the route each engine took for its from-scratch refresh
    assert got[1][0] == got[0][0]
    assert got[1][2] == got[0][2] >= 1               # the levels the workgroups found = the levels k_sched made
    assert got[1][0][-2] == po.Oracle(codes).score_tree(back)


def test_protein(mods):
    """the route serves 20-row tiles too: 33 taxa, rows of 32 words"""
    engine, po, synth, trees = mods
    n = 33
    letters, _ = synth.synth_alignment(n, 1000, "AA", 0.08, seed=7)
    codes = synth.letters_to_codes(letters, "AA")
    back = trees.random_topology(n, np.random.default_rng(8))
    got = {}
    for on in (0, 1):
        e = _engine(mods, codes, on, 8, datatype=engine.AA, plan_cache=0)
        assert e.get_option("kernel_states") == 20
        got[on] = _everything(e, back)
        e.close()
    assert got[1][1] == 1 and got[0][1] == 0
    assert got[1][0] == got[0][0]
    assert got[1][2] == got[0][2] >= 1
    assert got[1][0][-2] == po.Oracle(codes, datatype=engine.AA).score_tree(back)


@pytest.mark.parametrize("form", ["caterpillar", "balanced", "random"])
def test_tree_forms(mods, form):
    """200 taxa, rows of 32 words: the deepest level structure there is (a caterpillar: one or two records per level), the
    shallowest (fully balanced) and a random tree -- same results, and the same number of levels as k_sched reports"""
    engine, po, synth, trees = mods
    n = 200
    codes = _codes(mods, n, 32)
    back = {"caterpillar": _caterpillar, "balanced": _balanced}[form](trees, n) if form != "random" else trees.random_topology(n, np.random.default_rng(3))
    got = {}
    for on in (0, 1):
        e = _engine(mods, codes, on, plan_cache=0)
        got[on] = _everything(e, back)
        e.close()
    assert got[1][1] == 1 and got[0][1] == 0
    assert got[1][0] == got[0][0]
    assert got[1][2] == got[0][2] >= 1
    if form == "caterpillar":
        assert got[1][2] >= n - 3                    # (a path through every inner node)
    assert got[1][0][-2] == po.Oracle(codes).score_tree(back)


def _books(e):
    st = e.stats()
    return tuple(int(st[k]) for k in BOOKS)


@pytest.mark.parametrize("cache", [0, 1])
def test_state_across_calls(mods, cache):
    """one engine, many calls: two topologies in alternation, the same tree handed over again (plan cache on: the warm branch, the
    refresh replayed from the schedule a workgroup of the self-scheduled launch left behind), a sweep, an NNI step and a sweep (a partial refresh behind a self-scheduled
    one).  Results and, per from-scratch sweep, the books (view launches, refreshed vectors, plan and scan launches) equal the
    switch-off engine's"""
    engine, po, synth, trees = mods
    n = 40
    codes = _codes(mods, n, 32)
    rng = np.random.default_rng(11)
    A, B = trees.random_topology(n, rng), trees.random_topology(n, rng)
    got = {}
    for on in (0, 1):
        e = _engine(mods, codes, on, 8, plan_cache=cache)
        res = []
        prev = None
        for back in (A, B, A, B, A, B, B, B, A):     # six alternating steps, then the same tree again, twice
            before = _books(e)
            e.set_tree(back)
            k, best = e.sweep_scan(1, 6)
            after = _books(e)
            # (the same tree again with the plan cache on replays the schedule that the self-scheduled refresh left: k_newview_wgq)
            assert e.get_option("refresh_self_sched_active") == (on if cache == 0 or back is not prev else 0)
            prev = back
            res.append((int(k), int(best), tuple(a - b for a, b in zip(after, before))))
            res.append(e.score_tree())
        e.set_tree(A)
        res.append(_sweep(e, 6))
        res.append(e.optimize_nni(1, True, 2))
        res.append(e.get_tree().tolist())
        res.append(_sweep(e, 6))
        res.append(e.score_tree())
        ptn, tot = e.pattern_scores()
        res.append((int(tot), ptn.tolist()))
        got[on] = res
        e.close()
    assert got[1] == got[0]
    # one refresh launch and one planned scan per from-scratch sweep, all 3 (n - 2) vectors
    assert got[1][0][2][0] == 1 and got[1][0][2][1] == 3 * (n - 2)


@pytest.mark.parametrize("opts", [{"words_per_lane": 2}, {"views_mode": 0}, {"dev_sched": 0}])
def test_other_routes_stay(mods, opts):
    """what the route does not serve takes the routes of before: same results with the switch on and off, and the switch-on engine
    says that its from-scratch refresh was not self-scheduled"""
    engine, po, synth, trees = mods
    n = 33
    codes = _codes(mods, n, 96)
    back = trees.random_topology(n, np.random.default_rng(5))
    got = {}
    for on in (0, 1):
        e = _engine(mods, codes, on, **opts)
        got[on] = _everything(e, back)
        e.close()
    assert got[1][1] == 0 and got[0][1] == 0
    assert got[1][0] == got[0][0]
    assert got[1][0][-2] == po.Oracle(codes).score_tree(back)
