"""Re-weighting across row-pitch boundaries on LIVE engines.

A Fitch engine's row pitch Wp (Engine::pack) is the number of 32-site words of the weighted informative sites, rounded up to 32
words: every set_weights can move it, and with it the size of the vector store, the offset of the word-major copy behind it (the
allocation only grows: the old, larger layout stays in memory behind the new one), the cached plans, the tracker's sample layout,
the climb's tile count and the tile width k_climb_many takes.  Here one engine -- or one batch of engines -- lives through weight
vectors on both sides of the boundaries at 1024, 2048 and 3072 sites, up AND down, and every observable of every call equals the
oracle's (and a fresh engine's where stated).  Exact integer equality everywhere; every test asserts the pitch, or the many-climb
width, it is about."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AMB = np.array([3, 5, 6, 7, 9, 10, 11, 12, 13, 14], dtype=np.uint8)


def _alignment(n, P, alphabet, seed, rate=0.1, const=0, ambiguity=True):
    """codes with ambiguity / unknown codes as test_gpu_fuzz.random_case makes them; `const` columns made constant"""
    from mpboot_amd import synth
    letters, _ = synth.synth_alignment(n, P, alphabet, rate, seed=seed)
    codes = synth.letters_to_codes(letters, alphabet).copy()
    rng = np.random.default_rng(seed)
    if ambiguity:
        m = rng.random(codes.shape)
        codes[m < 0.04] = 22 if alphabet == "AA" else 15
        k = (m >= 0.04) & (m < 0.08)
        if alphabet == "AA":
            codes[(m >= 0.04) & (m < 0.06)] = 20 + rng.integers(0, 2)
        else:
            codes[k] = AMB[rng.integers(0, len(AMB), size=int(k.sum()))]
    if const:
        for j in rng.choice(P, size=const, replace=False):
            codes[:, j] = codes[0, j] if not ambiguity else (0 if alphabet == "AA" else 1)
    return codes


def _weights(total, counted, seed):
    """a weight vector whose entries over `counted` (a 0/1 mask: the patterns the packing keeps) sum to exactly `total`: a seeded set
    of zero weights, one heavy pattern (a tenth of the sites), the rest spread evenly and topped up one by one"""
    rng = np.random.default_rng(seed)
    P = len(counted)
    w = rng.integers(0, 4, size=P).astype(np.int64)          # (patterns the packing drops: any weight, zero included)
    idx = np.nonzero(np.asarray(counted) != 0)[0]
    live = rng.permutation(idx[rng.random(len(idx)) >= 0.15])
    w[idx] = 0
    heavy = max(1, total // 10)
    w[live[0]] = heavy
    rest, m = total - heavy, len(live) - 1
    w[live[1:]] = rest // m
    w[live[1:1 + rest % m]] += 1
    assert int(w[idx].sum()) == total and (w[idx] == 0).any() and int(w.max()) >= heavy
    return w.astype(np.int32)


def _pitch(e):
    wp = ((e.W + 31) // 32) * 32
    assert wp == e.Wp
    return wp


def _climb_both(e, o, tree, seed, radius=6):
    from mpboot_amd import engine
    for x in (e, o):
        x.set_tree(tree)
        x.seed_ties(engine.TIE_RANDOM, seed)
    o.trace(True)
    assert e.optimize_spr(1, radius) == o.optimize_spr(1, radius)
    assert [a.tolist() for a in e.moves()] == [a.tolist() for a in o.get_moves()]
    assert (e.get_tree() == o.get_tree()).all()
    assert e.tie_state() == o.tie_state()
    return len(e.moves()[0])


def _ladder(codes, aa, keep_all, sums, pitches, climb_steps, opts, seed):
    """one engine and one oracle through the weight vectors `sums`; after every set_weights the calls of test_gpu_stateful's
    operations 0, 1, 2 and 6, at `climb_steps` (counted from 1) a climb from a new random tree"""
    from mpboot_amd import engine, trees
    from oracle import pyoracle as po
    n, P = codes.shape
    dt_e, dt_o = (engine.AA, po.AA) if aa else (engine.DNA, po.DNA)
    rng = np.random.default_rng(seed)
    w0 = np.ones(P, dtype=np.int32)
    e = engine.FitchEngine(codes, w0, datatype=dt_e, keep_all=keep_all)
    o = po.Oracle(codes, w0, datatype=dt_o, keep_all=keep_all)
    for k, v in opts.items():
        e.set_option(k, v)
    counted = e.informative()
    assert counted.tolist() == o.informative().tolist()
    assert bool((counted != 0).all()) == keep_all
    known = [trees.random_topology(n, rng), trees.random_topology(n, rng)]
    for x in (e, o):
        x.set_tree(known[0])
        x.seed_ties(engine.TIE_RANDOM, seed)
    maxtrav = 6
    moved = 0
    seen = []
    for step, (total, want_wp) in enumerate(zip(sums, pitches), start=1):
        w = _weights(total, counted, 100 * seed + step)
        for x in (e, o):
            x.set_weights(w)
        assert (e.W, e.num_informative) == (o.W, o.num_informative), step
        assert _pitch(e) == want_wp, (step, total)
        seen.append(_pitch(e))
        if not opts and not aa:
            assert e.get_option("refresh_wm_active") == 1
        # the tree already set, under the new packing
        cur = o.score_tree()
        assert e.score_tree() == cur, step
        # a tree seen at an earlier step (its plans were made under another packing)
        t = known[(step * 7) % len(known)]
        assert e.score_tree(t) == o.score_tree(t), step
        # per-pattern lengths
        o.enable_persite(True)
        assert e.score_tree() == o.score_tree(), step
        pe, te = e.pattern_scores()
        po_, to = o.pattern_scores()
        assert te == to and pe.tolist() == po_.tolist(), step
        # one prune node's candidates
        rec = int(o.nodep()[1 + int(rng.integers(0, 2 * n - 2))])
        cur = o.score_tree()
        assert e.score_tree() == cur, step
        o.set_best(cur)
        o.trace(True)
        saved = o.get_tree().copy()
        o.rearrange(rec, 1, maxtrav)
        tq, tm = o.get_trace()
        keep = tq >= 0
        assert (o.get_tree() == saved).all()
        q, mp, _ = e.spr_scan(rec, 1, maxtrav)
        assert q.tolist() == tq[keep].tolist() and mp.tolist() == tm[keep].tolist(), step
        for x in (e, o):
            x.seed_ties(engine.TIE_RANDOM, seed + step)
        # a whole sweep: the best candidate
        cur = o.score_tree()
        assert e.score_tree() == cur, step
        _ntests, best = e.sweep_scan(1, maxtrav)
        lo = None
        for r in o.nodep()[1:2 * n - 1]:
            o.set_best(cur)
            o.trace(True)
            o.rearrange(int(r), 1, maxtrav)
            tq, tm = o.get_trace()
            if (tq >= 0).any():
                m = int(tm[tq >= 0].min())
                lo = m if lo is None else min(lo, m)
        assert lo is not None and best == lo, step
        for x in (e, o):
            x.seed_ties(engine.TIE_RANDOM, seed + 50 + step)
        if step in climb_steps:
            moved += _climb_both(e, o, trees.random_topology(n, rng), seed + 1000 + step)
            known.append(e.get_tree().copy())
            if opts.get("climb_device") == 2:
                assert e.stats()["climb_launches"] >= 1
    assert seen == list(pitches) and moved > 0
    assert e.score_tree() == o.score_tree()


LADDER_SUMS = [1000, 1024, 1025, 2048, 2049, 3100, 1025, 33, 1024, 2049]
LADDER_WP = [32, 32, 64, 64, 96, 128, 64, 32, 32, 96]
LADDER_OPTS = [{}, {"plan_cache": 0}, {"words_per_lane": 2}, {"views_mode": 1, "scan_batch": 2}, {"scan_prog": 2, "split_below": 0, "scan_batch": 64},
               {"refresh_wm": 0}, {"climb_device": 2, "climb_tile": 1}, {"climb_device": 2, "climb_tile": 4, "climb_groups": 2}]


@pytest.mark.parametrize("opts", LADDER_OPTS, ids=["-".join("%s%d" % kv for kv in o.items()) or "default" for o in LADDER_OPTS])
def test_pitch_ladder_dna(opts):
    """32 -> 64 -> 96 -> 128 words and down again to 32, then up to 96: the store grows three times and is then used at every smaller
    layout, the word-major copy's offset moving inside it"""
    codes = _alignment(24, 600, "DNA", 11)
    _ladder(codes, False, True, LADDER_SUMS, LADDER_WP, (3, 6, 7, 10), opts, 21)


@pytest.mark.parametrize("opts", [{}, {"views_mode": 1, "scan_batch": 2}], ids=["default", "views_mode1"])
def test_pitch_ladder_protein(opts):
    codes = _alignment(20, 300, "AA", 12)
    _ladder(codes, True, True, [1000, 1025, 2049, 1000], [32, 64, 96, 32], (2, 4), opts, 22)


def test_pitch_ladder_informative_sites_only():
    """keep_all = False: constant columns carry weight but no site -- the sums that set the pitch run over the informative patterns"""
    codes = _alignment(24, 600, "DNA", 13, const=60)
    _ladder(codes, False, False, [1000, 1025, 2049, 3100, 33, 1025], [32, 64, 96, 128, 32, 64], (2, 4, 6), {}, 23)


@pytest.mark.parametrize("copies,want_wp", [(2, 32), (4, 64), (6, 96)])
def test_weightless_patterns_behind_a_row_filled_to_its_last_site(copies, want_wp):
    """512 patterns at weight 2, 4, 6 fill rows of 32, 64, 96 words to the last bit; the 88 patterns behind them are kept
    (keep_all) at weight 0 and have no site: their per-pattern length is that of the site behind the last one, which does not
    exist here -- 0, not the word next door (the ladder's second step found k_pattern_sum reading it)"""
    from mpboot_amd import engine, trees
    from oracle import pyoracle as po
    codes = _alignment(24, 600, "DNA", 11)
    w = np.zeros(600, dtype=np.int32)
    w[:512] = copies
    e = engine.FitchEngine(codes, keep_all=True)
    o = po.Oracle(codes, keep_all=True)
    t = trees.random_topology(24, np.random.default_rng(1))
    for x in (e, o):
        x.set_weights(w)
        x.set_tree(t)
    assert _pitch(e) == want_wp and e.W == want_wp == o.W
    o.enable_persite(True)
    assert e.score_tree() == o.score_tree()
    pe, te = e.pattern_scores()
    po_, to = o.pattern_scores()
    assert te == to and pe.tolist() == po_.tolist()
    assert not pe[512:].any() and pe[:512].any()


@pytest.mark.parametrize("mulhits", [False, True], ids=["default", "mulhits"])
def test_tracked_climbs_across_a_pitch_change(mulhits):
    """-bb with the ratchet: a climb on the attach-time weights (32 words), one on ratchet weights half as many sites again (64 words:
    the tracker lays its sample weights out again by the sites of the new packing), one on the attach-time weights again"""
    from mpboot_amd import engine, trees
    from oracle import pyoracle as po
    n, P, B = 30, 800, 8
    codes = _alignment(n, P, "DNA", 14)
    rng = np.random.default_rng(24)
    w0 = _weights(1000, np.ones(P, dtype=np.int32), 240)
    e = engine.FitchEngine(codes, w0, keep_all=True)
    o = po.Oracle(codes, w0, keep_all=True)
    assert _pitch(e) == 32
    # the ratchet only adds copies (alignment.cpp:1915-1969): no attach-time pattern loses its last site
    w_r = (w0 + rng.multinomial(500, (w0 > 0) / (w0 > 0).sum())).astype(np.int32)
    assert int(w_r.sum()) == 1500 and not ((w0 > 0) & (w_r <= 0)).any()
    samples = rng.multinomial(1000, w0 / w0.sum(), size=B).astype(np.uint16)
    for x in (e, o):
        x.set_tree(trees.random_topology(n, np.random.default_rng(3)))
        x.seed_ties(engine.TIE_RANDOM, 5)
        x.ufboot_attach(samples)
        if mulhits:
            x.ufboot_set_mulhits(True)
    moved, booked = 0, []
    for it, (w, want_wp) in enumerate(((w0, 32), (w_r, 64), (w0, 32)), start=1):
        for x in (e, o):
            x.set_weights(w)
            x.ufboot_set_iteration(it)
        assert _pitch(e) == want_wp and e.W == o.W, it
        o.trace(True)
        assert e.optimize_spr(1, 6) == o.optimize_spr(1, 6), it
        assert [a.tolist() for a in e.moves()] == [a.tolist() for a in o.get_moves()], it
        assert (e.get_tree() == o.get_tree()).all(), it
        moved += len(e.moves()[0])
        assert [a.tolist() for a in e.ufboot_state()] == [a.tolist() for a in o.ufboot_state()], it
        assert e.ufboot_tree_logl().tolist() == o.ufboot_tree_logl().tolist(), it
        assert e.ufboot_counters()["tie_draws"] == o.ufboot_draws(), it
        assert e.ufboot_duplicates() == o.ufboot_duplicates(), it
        assert e.tie_state() == o.tie_state(), it
        if mulhits:
            for b in range(B):
                assert e.ufboot_sample_trees(b) == o.ufboot_sample_trees(b), (it, b)
        booked.append(len(o.ufboot_tree_logl()))
    assert moved > 0 and 0 < booked[0] < booked[1] and o.ufboot_bad() == 0          # (the ratchet climb was booked too)


# ---- many-climb rounds with mixed tile widths ------------------------------------------------------------------------------------
N_MANY, P_MANY = 40, 1200


@pytest.fixture(scope="module")
def many_case():
    from mpboot_amd import engine
    codes = _alignment(N_MANY, P_MANY, "DNA", 15, rate=0.15)
    e = engine.FitchEngine(codes)
    counted = e.informative()
    wA, wB = _weights(2000, counted, 31), _weights(2100, counted, 32)
    e.set_weights(wA)
    assert _pitch(e) == 64 and e.get_option("climb_tile_many") == 4
    e.set_weights(wB)
    assert _pitch(e) == 96 and e.get_option("climb_tile_many") == 2
    return dict(codes=codes, wA=wA, wB=wB, ref={})


def _setup(e, w, tree, seed):
    from mpboot_amd import engine
    e.set_weights(w)
    e.seed_ties(engine.TIE_RANDOM, seed)
    e.reset_node_order()
    e.set_tree(tree)


def _reference(case, which, tree_seed, seed, opts=None):
    """(score, moves, tree, tie state) of one climb: a fresh engine's solo mpf_optimize_spr, equal to the oracle's; computed once per
    (weights, tree, seed) and shared"""
    from mpboot_amd import engine, trees
    from oracle import pyoracle as po
    key = (which, tree_seed, seed, tuple(sorted((opts or {}).items())))
    if key not in case["ref"]:
        t = trees.random_topology(N_MANY, np.random.default_rng(tree_seed))
        s = engine.FitchEngine(case["codes"])
        for k, v in (opts or {}).items():
            s.set_option(k, v)
        _setup(s, case[which], t, seed)
        sig = (s.optimize_spr(1, 6), [x.tolist() for x in s.moves()], s.get_tree().tolist(), s.tie_state())
        o = po.Oracle(case["codes"], case[which])
        o.seed_ties(po.TIE_RANDOM, seed)
        o.reset_nodep()
        o.set_tree(t)
        o.trace(True)
        so = o.optimize_spr(1, 6)
        assert sig == (so, [x.tolist() for x in o.get_moves()], o.get_tree().tolist(), o.tie_state())
        case["ref"][key] = sig
    return case["ref"][key]


def _signature(e, score):
    return (int(score), [x.tolist() for x in e.moves()], e.get_tree().tolist(), e.tie_state())


def _run_out(batch):
    rounds = 0
    while batch.active():
        batch.round()
        rounds += 1
        assert rounds < 500
    return rounds


@pytest.mark.parametrize("going,starter,late", [("wA", "wB", 0), ("wB", "wA", 0), ("wA", "wB", 3)],
                         ids=["narrow_starter_at_0", "wide_starter_at_0", "narrow_starter_last"])
def test_a_mismatched_starter_beside_continuing_climbs(many_case, going, starter, late):
    """Three climbs are under way on one tile width when a fourth engine -- at index 0: the engine whose shape the launch used to
    take; or last -- is re-weighted across a pitch boundary and starts on the other width.  The continuing climbs keep the launch
    they were laid out for, the starter runs alone; every climb equals its solo run."""
    from mpboot_amd import engine, trees
    c = many_case
    width = {"wA": 4, "wB": 2}
    engs = [engine.FitchEngine(c["codes"]) for _ in range(4)]
    for e in engs:
        e.set_option("many_moves_cap", N_MANY // 2)
    early = [k for k in range(4) if k != late]
    for k in early:
        _setup(engs[k], c[going], trees.random_topology(N_MANY, np.random.default_rng(50 + k)), 70 + k)
        assert engs[k].get_option("climb_tile_many") == width[going]
    batch = engine.ClimbBatch(engs, 1, 6)
    for k in early:
        batch.start(k)
    batch.round()
    continuing = [k for k in early if batch.state[k] == 2]
    assert len(continuing) >= 1 and batch.active() == len(continuing)
    _setup(engs[late], c[starter], trees.random_topology(N_MANY, np.random.default_rng(50 + late)), 70 + late)
    assert engs[late].get_option("climb_tile_many") == width[starter] != width[going]
    assert _pitch(engs[late]) != _pitch(engs[continuing[0]])
    batch.start(late)
    _run_out(batch)
    for k in range(4):
        assert _signature(engs[k], batch.scores[k]) == _reference(c, starter if k == late else going, 50 + k, 70 + k), k
        assert engs[k].score_tree() == int(batch.scores[k]), k
    for k in continuing:
        assert engs[k].stats()["climb_launches"] >= 2, k


def test_an_engine_listed_twice_is_refused_by_the_round(many_case):
    from mpboot_amd import engine, trees
    c = many_case
    a = engine.FitchEngine(c["codes"])
    _setup(a, c["wA"], trees.random_topology(N_MANY, np.random.default_rng(50)), 70)
    with pytest.raises(engine.MpfError):
        batch = engine.ClimbBatch([a, a], 1, 6)
        batch.start(0)
        batch.start(1)
        batch.round()
    assert (a.get_tree() == trees.random_topology(N_MANY, np.random.default_rng(50))).all()
    assert a.optimize_spr(1, 6) == _reference(c, "wA", 50, 70)[0]


def test_weights_changed_in_the_middle_of_a_climb_are_refused(many_case):
    """set_weights between two rounds on an engine whose climb goes on: its tiles, scores and parameters were laid out for rows that
    no longer exist.  The round refuses before it touches anything; every engine of the batch is usable afterwards."""
    from mpboot_amd import engine, trees
    c = many_case
    engs = [engine.FitchEngine(c["codes"]) for _ in range(3)]
    for k, e in enumerate(engs):
        e.set_option("many_moves_cap", N_MANY // 2)
        _setup(e, c["wA"], trees.random_topology(N_MANY, np.random.default_rng(50 + k)), 70 + k)
    batch = engine.ClimbBatch(engs, 1, 6)
    for k in range(3):
        batch.start(k)
    batch.round()
    continuing = [k for k in range(3) if batch.state[k] == 2]
    assert continuing
    victim = continuing[-1]
    held = [e.get_tree().copy() for e in engs]
    engs[victim].set_weights(c["wB"])
    with pytest.raises(engine.MpfError):
        batch.round()
    assert [int(s) for s in batch.state] == [2 if k in continuing else 0 for k in range(3)]
    for k, e in enumerate(engs):
        assert (e.get_tree() == held[k]).all(), k
        f = engine.FitchEngine(c["codes"])
        f.set_weights(e.weights())
        assert e.score_tree() == f.score_tree(held[k]), k
        for x in (e, f):
            x.reset_node_order()
            x.seed_ties(engine.TIE_RANDOM, 90 + k)
        assert e.optimize_spr(1, 6) == f.optimize_spr(1, 6) and (e.get_tree() == f.get_tree()).all() and e.tie_state() == f.tie_state(), k


@pytest.mark.parametrize("at", [0, 1], ids=["first", "second"])
def test_climb_tile_set_on_one_engine_of_a_many_climb(many_case, at):
    """option climb_tile on one engine: its many-climb width is the option's, not the one the library picks -- it gives the launch its
    shape where it comes first (the others run alone) and runs alone otherwise; no launch error, the same climbs either way"""
    from mpboot_amd import engine, trees
    c = many_case
    engs = [engine.FitchEngine(c["codes"]) for _ in range(4)]
    engs[at].set_option("climb_tile", 1)
    for k, e in enumerate(engs):
        _setup(e, c["wA"], trees.random_topology(N_MANY, np.random.default_rng(50 + k)), 70 + k)
    assert [e.get_option("climb_tile_many") for e in engs] == [1 if k == at else 4 for k in range(4)]
    scores = engine.optimize_spr_many(engs, 1, 6)
    for k, e in enumerate(engs):
        assert _signature(e, scores[k]) == _reference(c, "wA", 50 + k, 70 + k, {"climb_tile": 1} if k == at else None), k
        assert e.stats()["climb_launches"] >= 1, k


def test_refinement_with_samples_on_both_sides_of_a_pitch_boundary():
    """refine_boot_trees(many_launch=True) on an alignment of exactly 1024 informative patterns: about half of the bootstrap samples
    pack into 32 words (32-word tiles in k_climb_many), the others into 64 (64-word tiles), nine engines take them as they come and
    every climb of two or more sweeps spans rounds (many_sweeps_inside 0) -- a finished engine is re-weighted to the other width and
    started beside climbs that go on.  Lengths and trees against IQTree::optimizeBootTrees' loop on the oracle."""
    from mpboot_amd import bootstrap, engine, shard, trees
    from oracle import pyoracle as po
    n, P, B, radius = 40, 1150, 48, 4
    codes = _alignment(n, P, "DNA", 31, rate=0.4, const=126, ambiguity=False)
    w0 = np.ones(P, dtype=np.int32)
    pool9 = [engine.FitchEngine(codes) for _ in range(9)]
    assert pool9[0].num_informative == 1024
    inf = pool9[0].informative() != 0
    samples = np.random.default_rng(5).multinomial(P, np.ones(P) / P, size=B).astype(np.uint16)
    infsum = samples[:, inf].astype(np.int64).sum(axis=1)
    assert int((infsum <= 1024).sum()) >= 12 and int((infsum > 1024).sum()) >= 12
    # the online phase's result, stood in for: every sample's tree = an SPR-optimal tree of ANOTHER sample's alignment
    o = po.Oracle(codes)
    boot_trees = []
    for b in range(B):
        o.set_weights(samples[(b * 7 + 3) % B].astype(np.int32))
        o.seed_ties(po.TIE_RANDOM, 100 + b)
        o.reset_nodep()
        o.set_tree(trees.random_topology(n, np.random.default_rng(b % 60)))
        o.optimize_spr(1, radius)
        boot_trees.append(o.get_tree().copy())
    for e in pool9:
        e.set_option("many_sweeps_inside", 0)
    widths = set()
    for b in (int(np.argmin(infsum)), int(np.argmax(infsum))):
        pool9[1].set_weights(samples[b].astype(np.int32))
        widths.add((_pitch(pool9[1]), pool9[1].get_option("climb_tile_many")))
    pool9[1].set_weights(w0)
    assert widths == {(32, 2), (64, 4)}
    sc, tr = bootstrap.refine_boot_trees(pool9, samples, boot_trees, 9, radius, batched=True, many_launch=True)
    moved = [0, 0]
    for b in range(B):
        o.set_weights(samples[b].astype(np.int32))
        o.seed_ties(po.TIE_RANDOM, shard.unit_seed(9, b))
        o.reset_nodep()
        o.set_tree(boot_trees[b])
        s = o.optimize_spr(1, radius)
        assert s == sc[b], b
        assert (o.get_tree() == tr[b]).all(), b
        moved[int(infsum[b] > 1024)] += int(not (o.get_tree() == boot_trees[b]).all())
    assert sum(moved) >= B // 2 and min(moved) >= 6          # the refinements really climb, on both widths
    assert all((x.weights() == w0).all() for x in pool9)
