"""TBR under -bb (mpf_ufboot_tbr_sweep / mpf_ufboot_optimize_tbr / mpf_tbr_pattern_terms on k_tbr_masks) against the witness in
tests/tbr_bb_witness.py: every entry of every visit's matrix through saveCurrentTree, in booking order.  There is no reference
function; the header states the semantics and the witness restates them from scratch.  Everything is compared exactly: integers
and the 64-bit state of the tie stream, no tolerance anywhere.  The inputs are those of tests/tbr_bb_cases.py, which
tests/test_tbr_bb_witness.py shows to exercise the update rule."""
import functools

import numpy as np
import pytest

import tbr_witness as tw
from helpers import load_fixture, same_topology
from oracle.search_slow import LONG_MAX
from tbr_bb_cases import CASES, DT, HANDOVER, handover_witness, make, run, setup

pytestmark = pytest.mark.gpu

BY_ID = {c["id"]: c for c in CASES}


def _engine(codes, weights, alphabet, keep_all=True, **kw):
    from mpboot_amd import engine
    return engine.FitchEngine(codes, weights, datatype=DT[alphabet], keep_all=keep_all, **kw)


def _code(fn):
    from mpboot_amd import engine
    with pytest.raises(engine.MpfError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def _same_books(e, w, n):
    assert e.ufboot_tree_logl().tolist() == w.treels_logl                                     # treels_logl, in order
    logl, counts, trees = e.ufboot_state()
    assert [-LONG_MAX if v <= -LONG_MAX / 2 else v for v in logl.tolist()] == w.boot_logl
    assert counts.tolist() == w.boot_counts
    if w.mulhits:
        for b in range(len(w.boot_sets)):
            assert e.ufboot_sample_trees(b) == sorted(w.boot_sets[b]), b
            for t in w.boot_sets[b]:
                assert same_topology(e.ufboot_tree(t), w.topologies[t], n)
    else:
        assert trees.tolist() == w.boot_trees
        for t in sorted(set(w.boot_trees)):
            if t >= 0:
                assert same_topology(e.ufboot_tree(t), w.topologies[t], n)
    if w.cutoff_from_btrees:
        assert e.ufboot_orig_logl().tolist() == w.boot_tree_orig_logl
    assert e.ufboot_counters()["tie_draws"] == w.ufb_draws
    assert e.tie_state() == int(w.rng.state)                                                 # the shared stream stands where the witness's does


@functools.lru_cache(maxsize=None)
def _witnessed(case_id):
    """a case run on the witness, once: (inputs, the witness behind its run, what the run returned)"""
    case = BY_ID[case_id]
    codes, weights, back, samples, radius, max_moves, w, cutoff = setup(case)
    want = run(case, w, radius, max_moves)
    return (codes, weights, back, samples, radius, max_moves, cutoff), w, want


def _attached(case, inputs, w, **options):
    from mpboot_amd import engine
    codes, weights, back, samples, _radius, _max_moves, cutoff = inputs
    e = _engine(codes, weights, case["alphabet"])
    for k, v in options.items():
        e.set_option(k, v)
    e.seed_ties(engine.TIE_RANDOM, 11 + case["seed"])
    e.set_tree(back)
    plain = e.tbr_sweep_best(inputs[4]) if case["kind"] == "sweep" else None
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
    assert [(int(x), int(y), int(z)) for x, y, z in zip(c, f, g)] == best and pairs == want_pairs
    # ... and what mpf_tbr_sweep_best gave on the same tree before the attach
    assert (c == plain[0]).all() and (f == plain[1]).all() and (g == plain[2]).all() and pairs == plain[3]
    assert (e.get_tree() == back).all()
    _same_books(e, w, n)
    assert e.get_option("tbr_booked") == len(w.calls) == pairs


def _climb_equals(e, w, want, radius, max_moves, n):
    assert e.ufboot_optimize_tbr(radius, max_moves) == want
    r, f, g, s = e.tbr_moves()
    assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(r, f, g, s)] == w.moves
    assert (e.get_tree() == np.array(w.back, dtype=np.int32)).all()
    _same_books(e, w, n)
    assert e.get_option("tbr_booked") == len(w.calls)


# ---------------------------------------------------------------- 1. every case against the witness
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tracked_sweep_and_climb_equal_the_witness(case):
    inputs, w, want = _witnessed(case["id"])
    codes, weights, back, _samples, radius, max_moves, _cutoff = inputs
    n = codes.shape[0]
    e, plain = _attached(case, inputs, w)
    if case["kind"] == "sweep":
        _sweep_equals(e, plain, w, want, radius, n, back)
    else:
        _climb_equals(e, w, want, radius, max_moves, n)
        assert want[1] >= 2
        # the tracked climb makes the plain climb's moves
        p = _engine(codes, weights, case["alphabet"])
        p.set_tree(back)
        assert p.optimize_tbr(radius, max_moves) == want
        assert all((a == b).all() for a, b in zip(p.tbr_moves(), e.tbr_moves()))
    assert e.get_option("tbr_book_batches") >= 1
    assert w.ufb_draws > 0 or w.mulhits


# ---------------------------------------------------------------- 2. batching and chunking change nothing
@pytest.mark.parametrize("chunk_vectors", (1, 0))
@pytest.mark.parametrize("book_rows", (1, 7, 0))
@pytest.mark.parametrize("case_id", ("dna-cut-sweep", "m32-default-sweep", "aa-mulhits-climb"))
def test_books_do_not_depend_on_the_batching(case_id, book_rows, chunk_vectors):
    """tbr_book_rows = 1 (an entry a batch), 7 (a batch ends in the middle of a row and of a visit: the matrices here have odd sides
    of 3 and more) and 0 (a chunk's entries in one batch), with every visit a chunk of its own and with the sweep in one chunk"""
    case = BY_ID[case_id]
    inputs, w, want = _witnessed(case_id)
    codes, _weights, back, _samples, radius, max_moves, _cutoff = inputs
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
def _weights_of(sites, rng):
    """weights 1 .. 5 that expand to exactly `sites` sites"""
    w = []
    while sum(w) < sites:
        w.append(min(int(rng.integers(1, 6)), sites - sum(w)))
    return np.array(w, dtype=np.int32)


# expanded site words: 1, 63, 64, 65 and 129 -- a row of one word, the two sides of the 64-word tile of a wave, and a third tile;
# the last word partly filled, and at 64 words full to its last bit
SITES = {1: 27, 63: 32 * 63 - 9, 64: 32 * 64, 65: 32 * 64 + 1, 129: 32 * 129 - 20}


@pytest.mark.parametrize("words", sorted(SITES))
@pytest.mark.parametrize("alphabet", ("dna", "aa", "m32"))
def test_mask_rows_are_the_witnesss_m(alphabet, words):
    from mpboot_amd import trees
    rng = np.random.default_rng(words)
    weights = _weights_of(SITES[words], rng)
    P = len(weights)
    assert -(-int(weights.sum()) // 32) == words
    shapes = set()
    for n in ((4, 6, 12) if words <= 63 else (4, 7)):
        codes, _ = tw.alignment(n, P, alphabet, 3 * words + n)
        for keep_all in (True, False):
            e = _engine(codes, weights, alphabet, keep_all)
            keep = np.ones(P, dtype=np.int64) if keep_all else np.asarray(e.informative()).astype(np.int64)
            wit = tw.TbrWitness(codes, weights, DT[alphabet])
            back = trees.random_topology(n, np.random.default_rng(n + words))
            length = e.score_tree(back)
            views = wit.views(back)
            for rec in [3 * t for t in range(1, n + 1)] + [3 * v + s for v in range(n + 1, 2 * n - 1) for s in range(3)]:
                for radius in ((1, 255) if n > 4 else (255,)):
                    q = int(back[rec])
                    rf = [views[q][0]] + wit.root_sets(back, views, q, radius)
                    rg = [views[rec][0]] + wit.root_sets(back, views, rec, radius)
                    nf, ng, terms = e.tbr_pattern_terms(rec, radius)
                    assert (1 + nf, 1 + ng) == (len(rf), len(rg)) == terms.shape[:2] and terms.shape[2] == P
                    shapes.add((len(rf) > 1, len(rg) > 1, rec // 3 <= n))
                    f, g, cost = e.tbr_scan(rec, radius)
                    for i in range(len(rf)):
                        want = ((rf[i][None, :] & np.stack(rg)) == 0) * keep[None, :]
                        assert (terms[i] == want).all(), (n, keep_all, rec, radius, i)
                        # the rows sum to the matrix: length(T_ij) = length(T) - M00 . w + Mij . w
                        assert ((terms[i].astype(np.int64) - terms[0, 0]) @ weights + length == cost[i]).all()
            assert (e.get_tree() == back).all()
            assert e.tbr_pattern_terms(3, 255, cap=0)[:2] == e.tbr_pattern_terms(3, 255)[:2]
    # a visit whose p is a tip (no G: a 1 x k matrix), one without F, and the 1 x 1 matrix of four taxa
    assert (True, False, True) in shapes and (False, True, False) in shapes and (False, False, False) in shapes and (True, True, False) in shapes


# ---------------------------------------------------------------- 4. hand-over
def test_spr_then_tbr_then_nni_on_one_tracker():
    """an SPR tracked climb, a TBR tracked climb and an NNI tracked climb on one tracker: each continues from the others' books"""
    from mpboot_amd import engine
    h = HANDOVER
    fx, samples, starts, w = handover_witness()
    n = fx["codes_np"].shape[0]
    e = engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"])
    e.seed_ties(engine.TIE_RANDOM, h["tie"])
    e.ufboot_attach(samples)
    e.set_tree(starts[0]); w.set_tree(starts[0])
    assert e.optimize_spr(1, h["spr_radius"]) == w.optimize(1, h["spr_radius"])
    _same_books(e, w, n)
    n1 = len(w.treels_logl)
    e.set_tree(starts[1]); w.set_tree(starts[1])
    calls0 = len(w.calls)
    _climb_equals_handover = e.ufboot_optimize_tbr(h["tbr_radius"], h["tbr_moves"])
    assert _climb_equals_handover == w.optimize_tbr(h["tbr_radius"], h["tbr_moves"])
    assert (e.get_tree() == np.array(w.back, dtype=np.int32)).all()
    _same_books(e, w, n)
    n2 = len(w.treels_logl)
    assert n2 > n1 > 0 and e.get_option("tbr_booked") == len(w.calls) - calls0
    e.set_tree(starts[2]); w.set_tree(starts[2])
    assert e.ufboot_optimize_nni(1, True) == w.optimize_nni(True)
    assert (e.get_tree() == np.array(w.back, dtype=np.int32)).all()
    _same_books(e, w, n)
    assert len(w.treels_logl) > n2


# ---------------------------------------------------------------- 5. served and refused
def test_a_suspended_tracker_books_nothing_and_moves_as_the_plain_climb():
    from mpboot_amd import engine
    case = BY_ID["dna-default-climb"]
    codes, weights, back, samples, radius, max_moves, _w, _cutoff = setup(case)
    e = _engine(codes, weights, "dna")
    e.seed_ties(engine.TIE_RANDOM, 5)
    e.ufboot_attach(samples)
    e.ufboot_set_ratchet_booking(False)
    e.set_weights((weights * 2).astype(np.int32))
    e.set_tree(back)
    state = e.tie_state()
    plain = make(codes, weights * 2, "dna", 1, None)
    plain.set_tree(back)
    want = plain.optimize_tbr(radius, max_moves)
    assert e.ufboot_optimize_tbr(radius, max_moves) == want and want[1] >= 2
    assert [tuple(int(x) for x in m) for m in zip(*e.tbr_moves())] == plain.moves
    assert (e.get_tree() == np.array(plain.back, dtype=np.int32)).all()
    c, f, g, pairs = e.ufboot_tbr_sweep(radius)
    best, want_pairs = plain.tbr_sweep(radius)
    assert [(int(x), int(y), int(z)) for x, y, z in zip(c, f, g)] == best and pairs == want_pairs
    assert len(e.ufboot_tree_logl()) == 0 and e.get_option("tbr_booked") == 0 and e.tie_state() == state


def test_refusals():
    from mpboot_amd import engine
    from nni_bb_cases import boot_samples, start_tree
    fx = load_fixture("dna_clean")
    w0 = fx["weights_np"]
    samples = boot_samples(len(fx["weights"]), 4, 5, fx["weights"])
    back = start_tree(fx, ("random", 0))

    def fresh(**kw):
        x = engine.FitchEngine(fx["codes_np"], w0, datatype=fx["datatype"], **kw)
        x.set_tree(back)
        return x

    def both(x):
        return (lambda: x.ufboot_tbr_sweep(2)), (lambda: x.ufboot_optimize_tbr(2, 2))

    e = fresh()
    for call in both(e):
        assert _code(call)[0] == -5                                      # no tracker
    e2 = engine.FitchEngine(fx["codes_np"], w0, datatype=fx["datatype"])
    e2.ufboot_attach(samples)
    for call in both(e2):
        assert _code(call)[0] == -5                                      # no tree
    e.ufboot_attach(samples)
    for call in both(e):
        assert _code(lambda: e.ufboot_tbr_sweep(0))[0] == -2 and _code(lambda: e.ufboot_optimize_tbr(256))[0] == -2
    # the old entry points still refuse a tracker, with the code and the text they had
    for call in (lambda: e.tbr_scan(3, 2), lambda: e.tbr_sweep_best(2), lambda: e.apply_tbr(3, -1, -1), lambda: e.optimize_tbr(2)):
        code, text = _code(call)
        assert code == -6 and "TBR is not served with a UFBoot tracker attached (nothing would be booked)" in text
    assert len(e.ufboot_tree_logl()) == 0

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
    # the weighted engine, with and without its plain TBR option
    cost = np.ones((4, 4), dtype=np.uint32) - np.eye(4, dtype=np.uint32)
    for opt in (0, 1):
        snk = fresh(cost=cost)
        snk.set_option("tbr_weighted", opt)
        snk.ufboot_attach(samples)
        for call in both(snk):
            code, text = _code(call)
            assert code == -6 and "weighted" in text
        assert len(snk.ufboot_tree_logl()) == 0
        assert _code(lambda: snk.tbr_pattern_terms(3, 2))[0] == -6
