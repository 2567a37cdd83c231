"""Parsimony branch lengths on the engine (mpf_branch_substitutions / mpf_branch_lengths on k_branch_subst and k_snk_branch_eval)
against the witness of PhyloTree::fixNegativeBranch in tests/brlen_witness.py.  Counts and weighted values are exact equality;
lengths are compared to 4 ulp (one log within 1 ulp and two divisions).

Size pin: 200 x 10 000 DNA and 120 x 3 000 protein, one random tree each; the witness takes about a second there."""
import numpy as np
import pytest

import brlen_witness as bw
import nni_snk_cases as cases
from helpers import FIXTURES, load_fixture
from nni_snk_witness import SnkScorer

pytestmark = pytest.mark.gpu

TAXA = (4, 5, 6, 16, 40)
COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)    # kept patterns: the tile edges of 32-bit (64 per wave) and 16-bit costs (128)
TILES = (-1, 0, 1, 2, 4)                                  # brlen_tile: the engine's choice, word-major copy, 1 | 2 | 4 words per lane
# sites of a Fitch engine (32 per word, 64 * vw words per tile): the tile edges of one, two and four words per lane
SITES = (2047, 2048, 2049, 4096, 4097, 8192, 8193, 16385)


def _alignment(n, P, protein, seed):
    """random tip codes with ambiguity and unknowns, weights 1 .. 5; keep_all engines keep every pattern"""
    rng = np.random.default_rng(seed)
    if protein:
        codes = rng.integers(0, 20, size=(n, P))
        odd = rng.integers(20, 23, size=(n, P))
    else:
        codes = 1 << rng.integers(0, 4, size=(n, P))
        odd = rng.integers(1, 16, size=(n, P))
    codes = np.where(rng.random((n, P)) < 0.1, odd, codes).astype(np.uint8)
    return codes, rng.integers(1, 6, size=P).astype(np.int32)


def _fitch(codes, weights, protein, keep_all=True):
    from mpboot_amd import engine
    return engine.FitchEngine(codes, weights, datatype=engine.AA if protein else engine.DNA, keep_all=keep_all)


def _got(eng, root=1):
    a, b, s = eng.branch_substitutions(root)
    return list(zip(a.tolist(), b.tolist())), s.astype(np.int64)


def _check(eng, order, want, root=1, what=None):
    got_order, got = _got(eng, root)
    assert got_order == order, what
    assert (got == want).all(), what


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_counts_equal_the_witness(protein, P):
    """every branch, pendant ones included, two roots, non-unit weights, every kernel shape"""
    from mpboot_amd import trees
    dt = 1 if protein else 0
    for n in TAXA:
        codes, weights = _alignment(n, P, protein, 100 * P + n)
        back = trees.random_topology(n, np.random.default_rng(n + P))
        eng = _fitch(codes, weights, protein)
        assert eng.num_informative == P
        eng.set_tree(back)
        for root in (1, n):
            order, want, _tot = bw.fitch_substitutions(codes, weights, dt, back, n, root)
            assert len(order) == 2 * n - 3
            for tile in TILES if not protein else (-1, 1):
                eng.set_option("brlen_tile", tile)
                _check(eng, order, want, root, (n, root, tile))
        assert (eng.get_tree() == back).all()


@pytest.mark.parametrize("sites", SITES)
def test_counts_at_the_tile_edges_of_every_width(sites):
    """DNA rows of more than one tile: the weights sum to `sites`, so the last word and the last tile are partly filled (or just
    full) for one, two and four words per lane; with and without 64-bit addressing (force_big: no word-major copy to read)"""
    from mpboot_amd import trees
    n, P = 16, 257
    codes, weights = _alignment(n, P, False, sites)
    weights = (weights + (sites - int(weights.sum())) // P).astype(np.int32)
    weights[-1] += sites - int(weights.sum())
    assert int(weights.sum()) == sites and weights.min() >= 1
    back = trees.random_topology(n, np.random.default_rng(sites))
    order, want = bw.fitch_substitutions_fast(codes, weights, 0, back, n, n)
    for big in (0, 1):
        eng = _fitch(codes, weights, False)
        eng.set_option("force_big", big)
        eng.set_tree(back)
        for tile in TILES:
            eng.set_option("brlen_tile", tile)
            _check(eng, order, want, n, (big, tile))


@pytest.mark.parametrize("keep_all", [False, True], ids=["informative", "keep_all"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(name, keep_all):
    """DNA, protein, binary and the multistate fixtures (20- and 32-row kernels); an engine that drops uninformative patterns counts
    the kept ones"""
    from mpboot_amd import engine, trees
    fx = load_fixture(name)
    codes, weights = fx["codes_np"], fx["weights_np"]
    n = codes.shape[0]
    eng = engine.FitchEngine(codes, weights, datatype=fx["datatype"], keep_all=keep_all)
    keep = None if keep_all else np.asarray(fx["informative"])
    back = trees.random_topology(n, np.random.default_rng(1))
    eng.set_tree(back)
    order, want, total = bw.fitch_substitutions(codes, weights, fx["datatype"], back, n, 1, keep=keep)
    _check(eng, order, want)
    assert (total == eng.score_tree(back)).all()


def test_counts_follow_set_weights():
    from mpboot_amd import trees
    n, P = 16, 129
    codes, weights = _alignment(n, P, False, 3)
    back = trees.random_topology(n, np.random.default_rng(3))
    eng = _fitch(codes, weights, False)
    eng.set_tree(back)
    order, want, _ = bw.fitch_substitutions(codes, weights, 0, back, n)
    _check(eng, order, want)
    w2 = np.random.default_rng(4).integers(0, 40, size=P).astype(np.int32)
    eng.set_weights(w2)
    order, want2, _ = bw.fitch_substitutions(codes, w2, 0, back, n)
    assert (want2 != want).any()
    _check(eng, order, want2)


@pytest.mark.parametrize("name", ["dna_48", "aa_40"])
def test_after_climbs_the_counts_are_a_fresh_engines(name):
    """an SPR climb and an NNI climb leave some views stale: the counts on the final tree equal a fresh engine's and the witness's;
    a second call launches once and refreshes nothing"""
    from mpboot_amd import engine, trees
    fx = load_fixture(name)
    codes, weights = fx["codes_np"], fx["weights_np"]
    n = codes.shape[0]
    eng = engine.FitchEngine(codes, weights, datatype=fx["datatype"])
    eng.set_tree(trees.random_topology(n, np.random.default_rng(2)))
    for climb in (lambda: eng.optimize_spr(1, 3), lambda: eng.optimize_nni(1, True, 3)):
        climb()
        final = eng.get_tree()
        order, got = _got(eng)
        fresh = engine.FitchEngine(codes, weights, datatype=fx["datatype"])
        fresh.set_tree(final)
        assert _got(fresh)[0] == order and (_got(fresh)[1] == got).all()
        w_order, want, _ = bw.fitch_substitutions(codes, weights, fx["datatype"], final, n, 1, keep=fx["informative"])
        assert w_order == order and (want == got).all()
        ops, launches = eng.stats()["newview_ops"], eng.get_option("brlen_launches")
        _check(eng, order, want)
        assert eng.stats()["newview_ops"] == ops and eng.get_option("brlen_launches") == launches + 1
        assert (eng.get_tree() == final).all()


def test_a_tracker_does_not_matter():
    from mpboot_amd import trees
    n, P = 16, 129
    codes, weights = _alignment(n, P, False, 8)
    back = trees.random_topology(n, np.random.default_rng(8))
    eng = _fitch(codes, weights, False)
    eng.set_tree(back)
    samples = np.random.default_rng(5).multinomial(P, np.ones(P) / P, size=4).astype(np.uint16)
    eng.ufboot_attach(samples)
    before = [x.tolist() for x in eng.ufboot_state()]
    order, want, _ = bw.fitch_substitutions(codes, weights, 0, back, n)
    _check(eng, order, want)
    assert [x.tolist() for x in eng.ufboot_state()] == before and (eng.get_tree() == back).all()


# ---------------------------------------------------------------- the weighted engine
def _weighted(codes, weights, protein, cost, keep_all=True):
    from mpboot_amd import engine
    return engine.FitchEngine(codes, weights, datatype=engine.AA if protein else engine.DNA, keep_all=keep_all, cost=cost)


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_weighted_values_equal_the_witness(protein, P):
    """the full length of the tree rooted at every branch in ParsTree::computeParsimonyBranch's orientation: 16-bit and 32-bit costs,
    symmetric and non-symmetric matrices, two roots"""
    from mpboot_amd import trees
    S = 20 if protein else 4
    for i, n in enumerate(TAXA):
        kind = ("metric", "asym")[(i + COUNTS.index(P)) % 2]
        cost = cases.cost_of(kind, S, seed=7 + i)
        codes, weights = _alignment(n, P, protein, 100 * P + n)
        back = trees.random_topology(n, np.random.default_rng(n + P))
        sc = SnkScorer(codes, weights, cost, protein=protein)
        eng = _weighted(codes, weights, protein, cost)
        assert eng.num_informative == P
        for short in (1, 0):
            eng.set_option("sankoff_short", short)
            eng.set_tree(back)
            for root in (1, n):
                order, want = bw.weighted_values(sc, back, n, root)
                _check(eng, order, want, root, (n, kind, short, root))
        assert (eng.get_tree() == back).all()


def test_weighted_asymmetric_orientation_shows():
    """(the committed case in which the orientation decides: inner branches differ, and the reversed orientation is another value)"""
    from mpboot_amd import trees
    fx = load_fixture("dna_ambig")
    n = fx["codes_np"].shape[0]
    cost = cases.cost_of("asym", 4)
    back = trees.random_topology(n, np.random.default_rng(0))
    sc = SnkScorer(fx["codes_np"], fx["weights_np"], cost)
    order, want = bw.weighted_values(sc, back, n, 1)
    _o, rev = bw.weighted_values(sc, back, n, 1, reverse=True)
    inner = [int(w) for (v1, v2), w in zip(order, want) if v1 > n and v2 > n]
    assert len(set(inner)) > 1 and (want != rev).any()
    eng = _weighted(fx["codes_np"], fx["weights_np"], False, cost, keep_all=False)
    eng.set_tree(back)
    _check(eng, order, want)


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_weighted_wide_addressing(protein):
    """option force_big: 64-bit pointers per row (BUF off)"""
    from mpboot_amd import trees
    n, P = 16, 129
    cost = cases.cost_of("asym", 20 if protein else 4)
    codes, weights = _alignment(n, P, protein, 5)
    back = trees.random_topology(n, np.random.default_rng(2))
    order, want = bw.weighted_values(SnkScorer(codes, weights, cost, protein=protein), back, n, 1)
    eng = _weighted(codes, weights, protein, cost)
    eng.set_option("force_big", 1)
    for short in (1, 0):
        eng.set_option("sankoff_short", short)
        eng.set_tree(back)
        _check(eng, order, want)


@pytest.mark.parametrize("name", ["morph32", "morph32_40"])
def test_weighted_32_state_kernels(name):
    """multistate data under a matrix runs the 32-row kernels; with a symmetric matrix every branch gives the tree's length, which
    the pinned oracle's weighted score_tree provides"""
    from mpboot_amd import engine, trees
    from oracle import pyoracle as po
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    cost = cases.metric(32, 4)
    o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
    eng = engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
    assert eng.get_option("kernel_states") == 32
    back = trees.random_topology(n, np.random.default_rng(1))
    want = o.score_tree(back)
    for short in (1, 0):
        eng.set_option("sankoff_short", short)
        eng.set_tree(back)
        order, got = _got(eng)
        assert order == bw.branch_order(back, n, 1)
        assert (got == want).all()


# ---------------------------------------------------------------- lengths
def _ulps(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))           # (positive doubles: the bit patterns are ordered)


def test_branch_lengths_fitch():
    """the formula on the engine's counts: a zero-count branch takes 1 / N, the 1e-6 floor, unit_cost_parstree"""
    from mpboot_amd import trees
    n, P = 16, 65
    codes, weights = _alignment(n, P, False, 11)
    back = trees.random_topology(n, np.random.default_rng(11))
    cherry = next([int(back[3 * v + s]) // 3 for s in range(3) if int(back[3 * v + s]) // 3 <= n] for v in range(n + 1, 2 * n - 1)
                  if sum(int(back[3 * v + s]) // 3 <= n for s in range(3)) == 2)
    codes[cherry[1] - 1] = codes[cherry[0] - 1]                  # two identical sister taxa ...
    eng = _fitch(codes, weights, False)
    eng.set_tree(back)
    order, subst, _ = bw.fitch_substitutions(codes, weights, 0, back, n)
    assert (subst == 0).any() and (subst > 0).any()              # ... leave their pendant branches without a change
    N = int(weights.sum())
    for n_sites in (N, 3 * N, 10 ** 7):
        a, b, got = eng.branch_lengths(n_sites)
        assert list(zip(a.tolist(), b.tolist())) == order
        want = bw.lengths(subst, n_sites, 4)
        assert (_ulps(got, want) <= 4).all()
    zero = subst == 0
    a, b, got = eng.branch_lengths(N)
    assert (_ulps(got[zero], bw.lengths([1], N, 4)[0]) <= 4).all()                   # the 1 / N rule
    assert (eng.branch_lengths(10 ** 7)[2][zero] == 1e-6).all()                      # the floor (1e-7 < MIN_BRANCH_LEN)
    tree_len = eng.score_tree(back)
    a, b, got = eng.branch_lengths(8 * tree_len, unit_cost_parstree=True)
    assert list(zip(a.tolist(), b.tolist())) == order
    assert (_ulps(got, bw.lengths([tree_len] * len(order), 8 * tree_len, 4)) <= 4).all()


def test_branch_lengths_protein_and_weighted():
    """S = 20 in the correction; a weighted engine puts the whole tree length over N: x <= 0 and the length stays uncorrected; the
    unit_cost_parstree flag is ignored there"""
    from mpboot_amd import trees
    n, P = 16, 65
    codes, weights = _alignment(n, P, True, 12)
    back = trees.random_topology(n, np.random.default_rng(12))
    eng = _fitch(codes, weights, True)
    eng.set_tree(back)
    order, subst, _ = bw.fitch_substitutions(codes, weights, 1, back, n)
    N = int(weights.sum())
    assert (_ulps(eng.branch_lengths(N)[2], bw.lengths(subst, N, 20)) <= 4).all()
    cost = cases.cost_of("asym", 20)
    snk = _weighted(codes, weights, True, cost)
    snk.set_tree(back)
    order, val = bw.weighted_values(SnkScorer(codes, weights, cost, protein=True), back, n, n)
    assert (val * 20 >= 19 * N).all()                            # x = 1 - (20 / 19) val / N <= 0
    a, b, got = snk.branch_lengths(N, n)
    assert list(zip(a.tolist(), b.tolist())) == order
    want = bw.lengths(val, N, 20)
    assert (want == val / np.float64(N)).all() and (_ulps(got, want) <= 4).all()
    assert (snk.branch_lengths(N, n, unit_cost_parstree=True)[2] == got).all()
    big = 40 * int(val.max())
    assert (_ulps(snk.branch_lengths(big, n)[2], bw.lengths(val, big, 20)) <= 4).all()


def test_what_is_refused():
    from mpboot_amd import engine, trees
    n, P = 16, 65
    codes, weights = _alignment(n, P, False, 13)
    eng = _fitch(codes, weights, False)
    with pytest.raises(engine.MpfError) as ei:                   # no tree
        eng.branch_substitutions()
    assert ei.value.code == -5                                   # MPF_E_STATE
    eng.set_option("grow_max_tips", 9)                           # (test aid: the stepwise addition stops at nine of sixteen tips)
    eng.stepwise_addition(5)
    for call in (lambda: eng.branch_substitutions(), lambda: eng.branch_lengths(100)):
        with pytest.raises(engine.MpfError) as ei:               # a partial tree
            call()
        assert ei.value.code == -5
    eng.set_option("grow_max_tips", 0)
    back = trees.random_topology(n, np.random.default_rng(13))
    eng.set_tree(back)
    for root in (0, n + 1):
        with pytest.raises(engine.MpfError):
            eng.branch_substitutions(root)
    with pytest.raises(engine.MpfError):
        eng.branch_lengths(0)
    with pytest.raises(engine.MpfError):
        eng.set_option("brlen_tile", 3)
    order, want, _ = bw.fitch_substitutions(codes, weights, 0, back, n)
    _check(eng, order, want)                                     # ... and served on the complete tree


@pytest.mark.parametrize("nt,L,alpha", [(200, 10000, "DNA"), (120, 3000, "AA")])
def test_counts_at_size(nt, L, alpha):
    from mpboot_amd import synth, trees
    letters, _ = synth.synth_alignment(nt, L, alpha, 0.08, seed=4)
    codes = synth.letters_to_codes(letters, alpha)
    protein = alpha == "AA"
    weights = np.ones(codes.shape[1], dtype=np.int32)
    back = trees.random_topology(nt, np.random.default_rng(5))
    order, want = bw.fitch_substitutions_fast(codes, weights, 1 if protein else 0, back, nt, 1)
    eng = _fitch(codes, weights, protein)
    eng.set_tree(back)
    _check(eng, order, want)
    if not protein:
        cost = cases.cost_of("asym", 4)
        order, want = bw.weighted_values(SnkScorer(codes, weights, cost), back, nt, 1)
        snk = _weighted(codes, weights, False, cost)
        snk.set_tree(back)
        _check(snk, order, want)
