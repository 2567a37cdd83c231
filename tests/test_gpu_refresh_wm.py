"""Refreshes on the word-major copy alone (option refresh_wm; k_newview_wgq / k_newview_chain / k_evaluate in their word-major
shapes, Engine::rows_ok_ and Engine::ensure_rows, mpboot_amd/csrc/kernels.hip and engine.cpp).

A DNA engine keeps every vector in two layouts.  With refresh_wm = 1 (the default) a refresh reads and writes the word-major copy
only and the rows are rewritten from it when a launch asks for them.  The reference of every comparison is the same engine with
refresh_wm = 0, the code path from before the option existed; where the CPU oracle serves a call it is asked too.  Integer work:
every comparison is exact.

Shapes: 5 taxa (one inner level) and 33 taxa (several levels, most of them narrower than one round of a workgroup: the clamped
surplus lanes), rows of 32, 96 and 1056 words with the refresh tile forced to 8 and 32 words, so that the tile count is below 8
(96 / 32 = 3, 32 / 8 = 4, 32 / 32 = 1), no multiple of 8 (96 / 8 = 12, 1056 / 8 = 132, 1056 / 32 = 33) -- the cases the kernel's
tile-to-XCD mapping splits unevenly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SITES = {32: 1000, 96: 3000, 1056: 33700}            # sites -> Wp = 32-site words, padded to a multiple of 32


@pytest.fixture(scope="module")
def mods():
    from mpboot_amd import engine, synth, trees
    from oracle import pyoracle as po
    return engine, po, synth, trees


_data = {}


def _alignment(mods, n, wp):
    """(codes, start tree) of a shape, made once per module"""
    engine, po, synth, trees = mods
    if (n, wp) not in _data:
        # (synth_alignment hands out DISTINCT patterns and five taxa have 4^5 = 1024 of them: wider rows repeat a block of 1000)
        base = min(SITES[wp], 1000) if n == 5 else SITES[wp]
        letters, _ = synth.synth_alignment(n, base, "DNA", 0.08, seed=100 * n + wp)
        codes = np.tile(synth.letters_to_codes(letters, "DNA"), (1, SITES[wp] // base))
        back = trees.random_topology(n, np.random.default_rng(n + wp))
        _data[(n, wp)] = (codes, back)
    return _data[(n, wp)]


def _engine(mods, codes, wm, tile=0, **opts):
    engine = mods[0]
    e = engine.FitchEngine(codes)
    e.set_option("refresh_wm", wm)
    if tile:
        e.set_option("views_tile", tile)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def _sweep(e, r):
    """everything a sweep of radius r reports: the timed call's (tests, best) and every candidate of the same sweep"""
    k, best = e.sweep_scan(1, r)
    n, mp, off = e.sweep_costs(1, r)
    return int(k), int(best), int(n), mp.tolist(), off.tolist()


@pytest.mark.parametrize("n,wp,tile", [(5, 32, 8), (5, 96, 32), (33, 32, 32), (33, 96, 8), (33, 96, 32), (33, 1056, 8), (33, 1056, 32)])
@pytest.mark.parametrize("cache", [1, 0])
def test_sweep_equals_the_row_major_engine(mods, n, wp, tile, cache):
    """set_tree; sweep_scan(1, r) for r = 1, 3, 6: test count, best score, every candidate score and score_tree equal the
    refresh_wm = 0 engine's, with check_counts on (host-planned sweep, counts verified) and off (the device-planned sweep that
    the benchmark times), plan cache on and off"""
    engine, po, synth, trees = mods
    codes, back = _alignment(mods, n, wp)
    got = {}
    for wm in (0, 1):
        res = []
        for check in (1, 0):
            e = _engine(mods, codes, wm, tile, plan_cache=cache, check_counts=check)
            assert e.Wp == wp
            assert e.get_option("refresh_wm") == wm and e.get_option("refresh_wm_active") == wm
            for r in (1, 3, 6):
                e.set_tree(back)
                res.append(_sweep(e, r))
                res.append(e.score_tree())
            res.append(e.score_tree(back))                       # from scratch, then the evaluate alone
            e.close()
        got[wm] = res
    assert got[1] == got[0]
    assert got[1][-1] == po.Oracle(codes).score_tree(back)


@pytest.mark.parametrize("n,wp,tile", [(33, 96, 8), (33, 1056, 32)])
def test_sweep_move_sweep(mods, n, wp, tile):
    """a move as trees.random_spr_moves applies it (a scan of one prune node on a tree just handed over: a partial, chained
    refresh), then the sweep of the new tree; and moves made inside the engine (an NNI step invalidates the vectors around the
    move only), so that the chained refresh reads word-major inputs while the rows are stale, then the sweep again"""
    engine, po, synth, trees = mods
    codes, back = _alignment(mods, n, wp)
    got = {}
    for wm in (0, 1):
        e = _engine(mods, codes, wm, tile)
        res = []
        b = trees.random_spr_moves(e, back, np.random.default_rng(9), 3)
        res.append(b.tolist())
        e.set_tree(b)
        res.append(_sweep(e, 6))
        if wm:
            assert e.get_option("rows_ok") == 0
        res.append(e.optimize_nni(1, True, 2))
        res.append(e.get_tree().tolist())
        res.append(_sweep(e, 6))
        res.append(e.score_tree())
        if wm:
            assert e.get_option("ensure_rows_launches") == 0     # every kernel on the way read the word-major copy
        got[wm] = res
        e.close()
    assert got[1] == got[0]


@pytest.mark.parametrize("n,wp,tile", [(5, 32, 8), (33, 96, 8), (33, 1056, 32)])
def test_rows_on_demand(mods, n, wp, tile):
    """after a word-major-only refresh a consumer of rows (per-pattern scores; the NNI evaluation on its row-major shape) gets
    them rewritten by ONE conversion launch; a second consumer finds them current"""
    engine, po, synth, trees = mods
    codes, back = _alignment(mods, n, wp)
    ref = _engine(mods, codes, 0, tile)
    e = _engine(mods, codes, 1, tile)
    for x in (ref, e):
        x.set_option("nni_tile", 1)                              # NNI scoring from the row-major store
        x.set_tree(back)
    want = tuple(int(v) for v in ref.sweep_scan(1, 3))
    assert tuple(int(v) for v in e.sweep_scan(1, 3)) == want
    assert ref.get_option("rows_ok") == 1 and ref.get_option("ensure_rows_launches") == 0
    stale = n >= 8                                               # (the device-planned sweep: refresh and planned scan, nothing reads rows;
    if stale:                                                    #  smaller trees take host-planned scans)
        assert e.get_option("rows_ok") == 0 and e.get_option("ensure_rows_launches") == 0
    before = e.get_option("ensure_rows_launches")
    ptn, tot = e.pattern_scores()
    rptn, rtot = ref.pattern_scores()
    assert tot == rtot and ptn.tolist() == rptn.tolist()
    assert tot == po.Oracle(codes).score_tree(back)
    assert e.get_option("rows_ok") == 1
    after = e.get_option("ensure_rows_launches")
    assert after == before + 1 if stale else after <= before + 1
    a, b, ln = e.nni_scores(1)
    ra, rb, rln = ref.nni_scores(1)
    assert a.tolist() == ra.tolist() and b.tolist() == rb.tolist() and ln.tolist() == rln.tolist()
    ptn2, tot2 = e.pattern_scores()
    assert tot2 == tot and ptn2.tolist() == ptn.tolist()
    assert e.get_option("ensure_rows_launches") == after          # no second conversion
    assert ref.get_option("ensure_rows_launches") == 0
    # a new from-scratch refresh makes the rows stale again, the NNI evaluation converts once more
    if stale:
        e.set_tree(back)
        assert tuple(int(v) for v in e.sweep_scan(1, 3)) == want
        assert e.get_option("rows_ok") == 0
        a2, b2, ln2 = e.nni_scores(1)
        assert ln2.tolist() == rln.tolist()
        assert e.get_option("ensure_rows_launches") == after + 1


@pytest.fixture(scope="module")
def c2(mods):
    engine, po, synth, trees = mods
    letters, _ = synth.workload("C2")
    codes = synth.letters_to_codes(letters, "DNA")
    return codes, trees.random_topology(codes.shape[0], np.random.default_rng(1))


@pytest.mark.parametrize("climb_device", [0, 1])
def test_whole_climb(mods, c2, climb_device):
    """optimize_spr of the benchmark's second configuration (200 taxa x 10 000 patterns) from a random topology: same score,
    moves and final tree with refresh_wm 0 and 1, on host-driven batches (chained refreshes between the scans, the rows stale
    from the first refresh on) and with the persistent kernel allowed"""
    engine, po, synth, trees = mods
    codes, back = c2
    got = {}
    for wm in (0, 1):
        e = _engine(mods, codes, wm, climb_device=climb_device)
        e.set_tree(back)
        e.seed_ties(engine.TIE_RANDOM, 1)
        s = e.optimize_spr(1, 6)
        mv = [m.tolist() for m in e.moves()]
        got[wm] = (s, mv, e.get_tree().tolist(), e.score_tree())
        e.close()
    assert got[1] == got[0]
    assert len(got[1][1][0]) > 300


def test_unaffected_engines_ignore_the_option(mods):
    """a protein engine and a weighted (-cost) engine have no word-major copy: refresh_wm is reported as not in force, their rows
    stay current and nothing is ever converted"""
    engine, po, synth, trees = mods
    n = 12
    back = trees.random_topology(n, np.random.default_rng(2))
    letters, _ = synth.synth_alignment(n, 400, "AA", 0.1, seed=3)
    aa = synth.letters_to_codes(letters, "AA")
    letters, _ = synth.synth_alignment(n, 400, "DNA", 0.1, seed=3)
    dna = synth.letters_to_codes(letters, "DNA")
    c = np.random.default_rng(1).integers(1, 5, size=(4, 4))
    cost = (np.triu(c, 1) + np.triu(c, 1).T).astype(np.uint32)
    cases = [(engine.FitchEngine(aa, datatype=engine.AA), po.Oracle(aa, datatype=po.AA)),
             (engine.FitchEngine(dna, cost=cost), po.Oracle(dna, cost=cost))]
    for e, o in cases:
        e.set_option("refresh_wm", 1)
        assert e.get_option("refresh_wm") == 1 and e.get_option("refresh_wm_active") == 0
        assert e.score_tree(back) == o.score_tree(back)
        k, mp, off = e.sweep_costs(1, 3)
        assert e.get_option("rows_ok") == 1 and e.get_option("ensure_rows_launches") == 0
        e.set_option("refresh_wm", 0)
        e.set_tree(back)
        k0, mp0, off0 = e.sweep_costs(1, 3)
        assert (k, mp.tolist()) == (k0, mp0.tolist())
        e.close()
