"""TBR under -bb on the weighted (-cost) engine (mpf_ufboot_tbr_sweep / mpf_ufboot_optimize_tbr / mpf_tbr_pattern_lengths on
k_tbr_snk_vals, options "tbr_weighted" and "tbr_weighted_tracked") against the witness in tests/tbr_snk_bb_witness.py: every entry of
every visit's matrix through saveCurrentTree, in booking order, each under its full weighted length with its own row of per-pattern
minima.  There is no reference function; the header states the semantics and the witness restates them from scratch.  Everything is
compared exactly: integers and the 64-bit state of the tie stream, no tolerance anywhere.  The inputs are those of
tests/tbr_snk_bb_cases.py, which tests/test_tbr_snk_bb_witness.py shows to exercise the update rule.

Every engine here sets tbr_weighted_tracked = 1: on an engine without the option this file fails."""
import functools

import numpy as np
import pytest

import tbr_witness as tw
from helpers import load_fixture
from nni_snk_cases import cost_of
from tbr_snk_bb_cases import BIG, BIG_SIZES, CASES, DT, HANDOVER, STATES, FormB, make, matrix_of, run, setup, visit_rows
from tbr_snk_bb_witness import RowScorer
from test_gpu_tbr_bb import _code, _same_books

pytestmark = pytest.mark.gpu

BY_ID = {c["id"]: c for c in CASES}


def _engine(codes, weights, alphabet, cost, keep_all=True, short=None, tracked=1, weighted=1):
    from mpboot_amd import engine
    e = engine.FitchEngine(codes, weights, datatype=DT[alphabet], keep_all=keep_all, cost=cost)
    e.set_option("tbr_weighted", weighted)
    e.set_option("tbr_weighted_tracked", tracked)
    assert e.get_option("tbr_weighted_tracked") == tracked
    if short is not None:
        e.set_option("sankoff_short", short)
        assert e.get_option("sankoff_packed") == short
    return e


@functools.lru_cache(maxsize=None)
def _witnessed(case_id):
    """a case run on the witness, once: (inputs, the witness behind its run, what the run returned)"""
    case = BY_ID[case_id]
    codes, weights, cost, back, samples, radius, max_moves, w, cutoff = setup(case)
    want = run(case, w, radius, max_moves)
    return (codes, weights, cost, back, samples, radius, max_moves, cutoff), w, want


def _attached(case, inputs, w, short=None, **options):
    from mpboot_amd import engine
    codes, weights, cost, back, samples, radius, _max_moves, cutoff = inputs
    e = _engine(codes, weights, case["alphabet"], cost, short=short)
    for k, v in options.items():
        e.set_option(k, v)
    e.seed_ties(engine.TIE_RANDOM, 11 + case["seed"])
    e.set_tree(back)
    plain = e.tbr_sweep_best(radius) if case["kind"] == "sweep" else None
    e.ufboot_attach(samples)
    if w.mulhits:
        e.ufboot_set_mulhits(True)
    if w.cutoff_from_btrees:
        e.ufboot_set_cutoff_from_btrees(True)
    if cutoff:
        e.ufboot_set_cutoff(cutoff)
    return e, plain


def _sweep_equals(e, plain, w, want, radius, n, back):
    c, f, g, pairs = e.ufboot_tbr_sweep(radius)
    best, want_pairs = want
    assert [(int(x), int(y), int(z)) for x, y, z in zip(c, f, g)] == [(int(x), y, z) for x, y, z in best] and pairs == want_pairs
    # ... and what mpf_tbr_sweep_best gave on the same tree before the attach
    assert (c == plain[0]).all() and (f == plain[1]).all() and (g == plain[2]).all() and pairs == plain[3]
    assert (e.get_tree() == back).all()
    _same_books(e, w, n)
    assert e.get_option("tbr_booked") == len(w.calls) == pairs


def _climb_equals(e, w, want, radius, max_moves, n):
    assert e.ufboot_optimize_tbr(radius, max_moves) == want
    r, f, g, s = e.tbr_moves()
    assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(r, f, g, s)] == [tuple(int(x) for x in m) for m in w.moves]
    assert (e.get_tree() == np.array(w.back, dtype=np.int32)).all()
    _same_books(e, w, n)
    assert e.get_option("tbr_booked") == len(w.calls)


# ---------------------------------------------------------------- 1. every case against the witness
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tracked_sweep_and_climb_equal_the_witness(case):
    """the 16-bit store; under the default rule the 32-bit store as well"""
    inputs, w, want = _witnessed(case["id"])
    codes, weights, cost, back, _samples, radius, max_moves, _cutoff = inputs
    n = codes.shape[0]
    for short in ((1, 0) if case["rule"] == "default" else (1,)):
        e, plain = _attached(case, inputs, w, short=short)
        if case["kind"] == "sweep":
            _sweep_equals(e, plain, w, want, radius, n, back)
        else:
            _climb_equals(e, w, want, radius, max_moves, n)
            assert want[1] >= 2
        assert e.get_option("tbr_book_batches") >= 1
    if case["kind"] == "climb":
        # the tracked climb makes the plain climb's moves, and stops at max_moves as it does
        p = _engine(codes, weights, case["alphabet"], cost)
        p.set_tree(back)
        assert p.optimize_tbr(radius, max_moves) == want
        assert all((a == b).all() for a, b in zip(p.tbr_moves(), e.tbr_moves()))
        assert want[1] <= max_moves
    assert w.ufb_draws > 0 or w.mulhits


# ---------------------------------------------------------------- 2. batching and chunking change nothing
@pytest.mark.parametrize("chunk_vectors", (1, 0))
@pytest.mark.parametrize("book_rows", (1, 7, 0))
@pytest.mark.parametrize("case_id", ("dna-cut-sweep", "m32-default-sweep", "aa-mulhits-climb"))
def test_books_do_not_depend_on_the_batching(case_id, book_rows, chunk_vectors):
    """tbr_book_rows = 1 (an entry a batch), 7 (a batch ends in the middle of a row and of a visit: the matrices here have odd sides
    of 3 and more) and 0 (the automatic cap: a chunk's entries in one batch), with every visit a chunk of its own and with the sweep
    in one chunk"""
    case = BY_ID[case_id]
    inputs, w, want = _witnessed(case_id)
    codes, _weights, _cost, back, _samples, radius, max_moves, _cutoff = inputs
    n = codes.shape[0]
    e, plain = _attached(case, inputs, w, tbr_book_rows=book_rows, tbr_chunk_vectors=chunk_vectors)
    if case["kind"] == "sweep":
        _sweep_equals(e, plain, w, want, radius, n, back)
        if chunk_vectors == 1:
            assert e.get_option("tbr_chunks") > 1
        if book_rows:
            assert e.get_option("tbr_book_batches") >= -(-want[1] // book_rows) > 1
        elif chunk_vectors == 0 and not w.cutoff:
            assert e.get_option("tbr_book_batches") == 1
    else:
        _climb_equals(e, w, want, radius, max_moves, n)


# ---------------------------------------------------------------- 3. the kernel's rows alone
# kept patterns -> elements of a row: in the 32-bit store one a pattern (1, 63, 64, 65, 129: a row of one element, the two sides of the
# 64-element tile of a wave, a third tile), in the 16-bit store one a PAIR (1 -> 1, 125 -> 63, 128 -> 64, 129 -> 65, 257 -> 129; the
# odd counts leave half a pair in the last element)
COUNTS = (1, 63, 64, 65, 125, 128, 129, 257)


def _records(n):
    return [3 * t for t in range(1, n + 1)] + [3 * v + s for v in range(n + 1, 2 * n - 1) for s in range(3)]


def _rows_equal(e, sc, back, weights, rec, radius, views, tag):
    F, G, want = visit_rows(sc, back, rec, radius, views)
    nf, ng, rows = e.tbr_pattern_lengths(rec, radius)
    assert rows.dtype == np.uint16 and (1 + nf, 1 + ng) == (1 + len(F), 1 + len(G)) == rows.shape[:2] and rows.shape[2] == len(weights), tag
    assert (rows == want).all(), tag
    f, g, cost = e.tbr_scan(rec, radius)
    assert f.tolist() == F and g.tolist() == G, tag
    # the rows sum to the matrix (dropped patterns read 0 and have no part in any length)
    kept = np.zeros(len(weights), dtype=np.int64)
    kept[sc.cols] = 1
    assert ((rows.astype(np.int64) * kept) @ np.asarray(weights, dtype=np.int64) == cost).all(), tag
    return rows


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("alphabet", ("dna", "aa", "m32"))
def test_rows_are_the_witnesss(alphabet, P):
    """every entry of every visit at 4 and 7 taxa, both stores, every pattern kept and the uninformative ones dropped; row 0 and
    column 0 read the resident vectors; [0][0] is the current tree's own row (mpf_nni_pattern_lengths' row 0, which
    launch_sankoff_pattern writes)"""
    from mpboot_amd import trees
    cost = matrix_of(alphabet, P)
    shapes = set()
    for n in (4, 7):
        codes, weights = tw.alignment(n, P, alphabet, 3 * P + n)
        back = trees.random_topology(n, np.random.default_rng(n + P))
        for keep_all in ((True, False) if P >= 63 else (True,)):
            e = _engine(codes, weights, alphabet, cost, keep_all)
            e.set_option("nni_weighted", 1)
            e.set_option("nni_weighted_tracked", 1)
            keep = np.ones(P, dtype=np.int64) if keep_all else np.asarray(e.informative()).astype(np.int64)
            sc = RowScorer(codes, weights * keep, DT[alphabet], cost)
            views = sc.views(back) if len(sc.cols) else None
            if views is None:
                continue                                  # (nothing kept: the engine has no pattern to score)
            for short in (1, 0):
                e.set_option("sankoff_short", short)
                e.set_tree(back)
                length = e.score_tree()
                current = e.nni_pattern_lengths(1)[3][0]
                for rec in _records(n):
                    for radius in ((1, 255) if n > 4 else (255,)):
                        rows = _rows_equal(e, sc, back, weights, rec, radius, views, (n, keep_all, short, rec, radius))
                        shapes.add((rows.shape[0] > 1, rows.shape[1] > 1, rec // 3 <= n))
                        assert (rows[0, 0] == current).all() and int(rows[0, 0].astype(np.int64) @ weights) == length
                assert (e.get_tree() == back).all()
                assert e.tbr_pattern_lengths(3, 255, cap=0)[:2] == e.tbr_pattern_lengths(3, 255)[:2]
    if P > 1:
        # a visit whose p is a tip (no G: a k x 1 ... 1 x k matrix), one without F, the 1 x 1 matrix of four taxa, and a full one
        assert (True, False, True) in shapes and (False, True, False) in shapes and (False, False, False) in shapes and (True, True, False) in shapes


@pytest.mark.parametrize("short", (1, 0))
def test_a_row_of_more_than_32_columns_splits_into_runs(short):
    """40 taxa at radius 6: a visit with more than 32 columns, so that a matrix row is two runs"""
    from mpboot_amd import trees
    n, P = 40, 65
    codes, weights = tw.alignment(n, P, "dna", 17)
    cost = cost_of("tstv", 4)
    back = trees.random_topology(n, np.random.default_rng(40))
    e = _engine(codes, weights, "dna", cost, short=short)
    e.set_tree(back)
    sc = RowScorer(codes, weights, 0, cost)
    views = sc.views(back)
    widths = {}
    for rec in _records(n):
        F, G = tw.lists(back, n, rec, 6)
        widths.setdefault(min((1 + len(G)) // 33, 1), (rec, 1 + len(F)))
    assert set(widths) == {0, 1}
    for k in (0, 1):
        rec = widths[k][0]
        rows = _rows_equal(e, sc, back, weights, rec, 6, views, (short, rec))
        assert (rows.shape[1] > 32) == (k == 1)
    assert widths[1][1] > 1


# ---------------------------------------------------------------- 4. hand-over
def test_spr_then_tbr_then_nni_on_one_tracker():
    """a weighted tracked SPR climb, a tracked TBR sweep and a weighted tracked NNI climb on one tracker: each continues from the
    others' books"""
    from mpboot_amd import engine
    from nni_bb_cases import boot_samples, start_tree
    from nni_snk_bb_witness import SnkNniBbWitness
    from tbr_snk_bb_witness import TbrSnkBbWitness

    class AllThree(SnkNniBbWitness, TbrSnkBbWitness):
        pass

    h = HANDOVER
    fx = load_fixture(h["fx"])
    n = fx["codes_np"].shape[0]
    cost = cost_of(h["cost"], 4)
    samples = boot_samples(len(fx["weights"]), h["B"], h["sseed"], fx["weights"])
    starts = [start_tree(fx, ("random", s)) for s in h["starts"]]
    w = AllThree(fx["codes_np"], fx["weights_np"], fx["datatype"], cost, h["tie"], samples, 1)
    w.took, w.memo = [], {}
    e = engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
    for opt in ("tbr_weighted", "tbr_weighted_tracked", "nni_weighted", "nni_weighted_tracked"):
        e.set_option(opt, 1)
    e.seed_ties(engine.TIE_RANDOM, h["tie"])
    e.ufboot_attach(samples)
    e.set_tree(starts[0]); w.set_tree(starts[0])
    assert e.optimize_spr(1, h["spr_radius"]) == w.optimize(1, h["spr_radius"])
    _same_books(e, w, n)
    n1 = len(w.treels_logl)
    e.set_tree(starts[1]); w.set_tree(starts[1])
    calls0 = len(w.calls)
    c, f, g, pairs = e.ufboot_tbr_sweep(h["tbr_radius"])
    best, want_pairs = w.tbr_sweep(h["tbr_radius"])
    assert [(int(x), int(y), int(z)) for x, y, z in zip(c, f, g)] == [(int(x), y, z) for x, y, z in best] and pairs == want_pairs
    _same_books(e, w, n)
    n2 = len(w.treels_logl)
    assert n2 > n1 > 0 and e.get_option("tbr_booked") == len(w.calls) - calls0 == pairs
    e.set_tree(starts[2]); w.set_tree(starts[2])
    w.edge = None
    assert e.ufboot_optimize_nni(1, True) == w.optimize_nni(True)
    assert (e.get_tree() == np.array(w.back, dtype=np.int32)).all()
    _same_books(e, w, n)
    assert len(w.treels_logl) > n2


# ---------------------------------------------------------------- 5. served and refused
def test_a_suspended_tracker_books_nothing_and_moves_as_the_plain_climb():
    from mpboot_amd import engine
    case = BY_ID["dna-default-climb"]
    codes, weights, cost, back, samples, radius, max_moves, _w, _cutoff = setup(case)
    e = _engine(codes, weights, "dna", cost)
    e.seed_ties(engine.TIE_RANDOM, 5)
    e.ufboot_attach(samples)
    e.ufboot_set_ratchet_booking(False)
    e.set_weights((weights * 2).astype(np.int32))
    e.set_tree(back)
    state = e.tie_state()
    plain = make(codes, weights * 2, "dna", cost, 1, None)
    plain.set_tree(back)
    want = plain.optimize_tbr(radius, max_moves)
    assert e.ufboot_optimize_tbr(radius, max_moves) == want and want[1] >= 2
    assert [tuple(int(x) for x in m) for m in zip(*e.tbr_moves())] == [tuple(int(x) for x in m) for m in plain.moves]
    assert (e.get_tree() == np.array(plain.back, dtype=np.int32)).all()
    c, f, g, pairs = e.ufboot_tbr_sweep(radius)
    best, want_pairs = plain.tbr_sweep(radius)
    assert [(int(x), int(y), int(z)) for x, y, z in zip(c, f, g)] == [(int(x), y, z) for x, y, z in best] and pairs == want_pairs
    assert len(e.ufboot_tree_logl()) == 0 and e.get_option("tbr_booked") == 0 and e.tie_state() == state


def test_refusals():
    from mpboot_amd import engine
    from nni_bb_cases import boot_samples, start_tree
    fx = load_fixture("dna_clean")
    w0 = fx["weights_np"]
    samples = boot_samples(len(fx["weights"]), 4, 5, fx["weights"])
    back = start_tree(fx, ("random", 0))
    tstv = cost_of("tstv", 4)

    def fresh(cost=tstv, weighted=1, tracked=1, **kw):
        x = engine.FitchEngine(fx["codes_np"], w0, datatype=fx["datatype"], cost=cost, **kw)
        x.set_option("tbr_weighted", weighted)
        x.set_option("tbr_weighted_tracked", tracked)
        x.set_tree(back)
        return x

    def both(x):
        return (lambda: x.ufboot_tbr_sweep(2)), (lambda: x.ufboot_optimize_tbr(2, 2))

    e = fresh()
    for call in both(e):
        assert _code(call)[0] == -5                                      # no tracker
    e.ufboot_attach(samples)
    assert _code(lambda: e.ufboot_tbr_sweep(0))[0] == -2 and _code(lambda: e.ufboot_optimize_tbr(256))[0] == -2
    # the five plain entries still refuse a tracker, with the code and the text they had
    for call in (lambda: e.tbr_scan(3, 2), lambda: e.tbr_sweep_best(2), lambda: e.apply_tbr(3, -1, -1), lambda: e.optimize_tbr(2)):
        code, text = _code(call)
        assert code == -6 and "TBR is not served with a UFBoot tracker attached (nothing would be booked)" in text
    assert len(e.ufboot_tree_logl()) == 0
    # option 0 (with the old message), and tbr_weighted 0 under tbr_weighted_tracked 1
    for weighted, tracked in ((1, 0), (0, 1), (0, 0)):
        x = fresh(weighted=weighted, tracked=tracked)
        x.ufboot_attach(samples)
        for call in both(x):
            code, text = _code(call)
            assert code == -6 and "the tracked TBR sweep is not served on the weighted (-cost) engine (its mask rows are Fitch joins)" in text
        assert _code(lambda: x.tbr_pattern_lengths(3, 2))[0] == -6
        assert len(x.ufboot_tree_logl()) == 0 and x.get_option("tbr_booked") == 0
    # a matrix that is not symmetric
    a = fresh(cost=cost_of("asym", 4))
    a.ufboot_attach(samples)
    for call in both(a) + (lambda: a.tbr_pattern_lengths(3, 2),):
        code, text = _code(call)
        assert code == -6 and "not symmetric" in text
    assert len(a.ufboot_tree_logl()) == 0

    def ratchet(x):
        pert, _st = engine.iq_perturb_weights(w0, fx["informative"], 50, 1, 12345)
        assert (pert != w0).any() and not ((w0 > 0) & (pert <= 0)).any()
        x.set_weights(pert)
        x.set_tree(back)

    named = [(lambda x: x.ufboot_set_store_trees(True), "-storetrees"),
             (lambda x: (x.ufboot_set_mulhits(True), x.ufboot_set_topboot(3)), "-mulhits -topboot"),
             (lambda x: x.ufboot_set_distinct_iter(2), "-distinct_iter_top_boot"),
             (ratchet, "ratchet")]
    for setter, word in named:
        x = fresh()
        x.seed_ties(engine.TIE_RANDOM, 3)
        x.ufboot_attach(samples)
        setter(x)
        state = x.tie_state()
        for call in both(x):
            code, text = _code(call)
            assert code == -6 and word in text, (word, text)
        assert len(x.ufboot_tree_logl()) == 0 and (x.get_tree() == back).all() and x.tie_state() == state
        assert x.get_option("tbr_booked") == 0
    # a sample-sharded tracker
    import ctypes as C
    ex = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)(lambda *a: 1)
    sh = fresh()
    sh.ufboot_attach(samples, shard=(0, 2), exchange=ex)
    for call in both(sh):
        code, text = _code(call)
        assert code == -6 and "sample-sharded" in text
    assert len(sh.ufboot_tree_logl()) == 0
    # a Fitch engine accepts the option, ignores it, serves its own tracked sweep and is refused the weighted diagnostic by name
    fe = engine.FitchEngine(fx["codes_np"], w0, datatype=fx["datatype"])
    fe.set_option("tbr_weighted_tracked", 1)
    assert fe.get_option("tbr_weighted_tracked") == 1
    fe.set_tree(back)
    code, text = _code(lambda: fe.tbr_pattern_lengths(3, 2))
    assert code == -6 and "weighted engines only" in text
    fe.ufboot_attach(samples)
    assert fe.ufboot_tbr_sweep(2)[3] > 0 and len(fe.ufboot_tree_logl()) > 0
    # mpf_tbr_pattern_terms stays Fitch only
    assert _code(lambda: e.tbr_pattern_terms(3, 2))[0] == -6


# ---------------------------------------------------------------- 6. above a single tile per row
def test_one_sweep_above_a_single_tile_per_row_with_20_states():
    """36 taxa x 260 protein patterns (130 elements a row in the 16-bit store: three tiles, the last of two elements), a random
    metric matrix, radius 2, 16 samples, one tracked sweep of 1382 entries, against the witness's vectorised form
    (tests/tbr_snk_bb_cases.py:FormB), which tests/test_tbr_snk_bb_witness.py ties to the from-scratch form row by row and book by
    book.  The witness's side takes about 0.2 s on one CPU core."""
    inputs_w = setup(BIG, cls=FormB, sizes=BIG_SIZES)
    codes, weights, cost, back, samples, radius, max_moves, w, cutoff = inputs_w
    want = run(BIG, w, radius, max_moves)
    n = codes.shape[0]
    assert n <= 40 and codes.shape[1] >= 2 * 129 and radius == 2 and len(samples) == 16
    e, plain = _attached(BIG, (codes, weights, cost, back, samples, radius, max_moves, cutoff), w, short=1)
    assert e.S == STATES["aa"]
    _sweep_equals(e, plain, w, want, radius, n, back)
    assert w.ufb_draws > 0 and w.final_trees_booked_as_interior() >= 1
