"""Multifurcating trees on the engine (mpf_polytomy_parsimony / mpf_polytomy_branch_substitutions / mpf_polytomy_branch_lengths on
k_poly_views and k_poly_snk_views) against the witnesses of tests/polytomy_witness.py.  Lengths of trees, _pattern_pars and subst
are exact equality; branch lengths are compared to 4 ulp (one log within 1 ulp and two divisions), as test_gpu_brlen.py does.

Size pin: 200 x 10 000 DNA with about a third of the inner branches contracted; the witness takes about a second there."""
import numpy as np
import pytest

import nni_snk_cases as cases
import polytomy_witness as pw

pytestmark = pytest.mark.gpu

TAXA = (4, 5, 6, 16, 40)
COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)    # kept patterns, the tile edges of the brlen tests
SITES = (2047, 2048, 2049, 4096, 4097, 8193)              # site totals of a Fitch engine, the tile edges of the brlen tests
BRLEN_TILES = (-1, 0, 1, 2, 4)
POLY_TILES = (0, 4, 8, 16, 32)


def _alignment(n, P, protein, seed):
    """random tip codes with 10 % ambiguity and unknowns, weights 1 .. 5 (as test_gpu_brlen.py generates them)"""
    rng = np.random.default_rng(seed)
    if protein:
        codes = rng.integers(0, 20, size=(n, P))
        odd = rng.integers(20, 23, size=(n, P))
    else:
        codes = 1 << rng.integers(0, 4, size=(n, P))
        odd = rng.integers(1, 16, size=(n, P))
    codes = np.where(rng.random((n, P)) < 0.1, odd, codes).astype(np.uint8)
    return codes, rng.integers(1, 6, size=P).astype(np.int32)


def _engine(codes, weights, protein, cost=None, keep_all=True):
    from mpboot_amd import engine
    return engine.FitchEngine(codes, weights, datatype=engine.AA if protein else engine.DNA, keep_all=keep_all, cost=cost)


def _parsimony_at(eng, root):
    """mpf_compute_parsimony_at on the engine's own tree: (length, _pattern_pars)"""
    import ctypes as C
    from mpboot_amd import engine
    s, ptn = C.c_uint32(), np.zeros(eng.P, dtype=np.uint16)
    rc = engine.load_library().mpf_compute_parsimony_at(eng.h, None, root, C.byref(s), ptn.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return int(s.value), ptn


def _ulps(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def _check(eng, wit, first, nbr, root, what=None, n_sites=None, patterns=True):
    """length, _pattern_pars, every branch's subst and length against the witness"""
    want_len, want_ptn = wit.parsimony(first, nbr, root)
    if patterns:
        got_len, got_ptn = eng.polytomy_parsimony(first, nbr, root, with_patterns=True)
        assert (got_ptn.astype(np.int64) == want_ptn).all(), what
    else:
        got_len = eng.polytomy_parsimony(first, nbr, root)
    assert got_len == want_len, what
    order, want = wit.substitutions(first, nbr, root)
    a, b, s = eng.polytomy_branch_substitutions(first, nbr, root)
    assert len(order) == eng.n + len(first) - 2
    assert list(zip(a.tolist(), b.tolist())) == order, what
    assert (s.astype(np.int64) == want).all(), what
    if n_sites:
        a, b, ln = eng.polytomy_branch_lengths(first, nbr, n_sites, root)
        assert list(zip(a.tolist(), b.tolist())) == order, what
        assert (_ulps(ln, pw.branch_lengths(want, n_sites, wit.S)) <= 4).all(), what


def _shapes(n, seed):
    """trees of n taxa: random collapses, the star, two adjacent polytomies, a polytomy at the root leaf's neighbour"""
    from mpboot_amd import trees
    rng = np.random.default_rng(seed)
    back = trees.random_topology(n, rng)
    out = [pw.random_collapse(back, n, rng, f) for f in (0.0, 0.35, 0.7)] + [pw.star(n)]
    if n >= 6:
        r0 = int(back[3]) // 3                              # the neighbour of leaf 1: contract every inner branch at it ...
        at_r0 = [(r0, int(back[3 * r0 + s]) // 3) for s in range(3) if int(back[3 * r0 + s]) // 3 > n]
        out.append(trees.collapse_branches(back, n, at_r0))
        inner = [(v, int(back[3 * v + s]) // 3) for v in range(n + 1, 2 * n - 1) for s in range(3) if int(back[3 * v + s]) // 3 > v]
        a, b = inner[len(inner) // 2]                       # ... and, around one kept branch, the branches at both its ends: two adjacent polytomies
        around = [br for br in inner if br != (a, b) and (a in br or b in br)]
        out.append(trees.collapse_branches(back, n, around))
    return out


# ---------------------------------------------------------------- the Fitch engine
@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_fitch_equals_the_witness(protein, P):
    """every shape of tree, roots 1 and n, non-unit weights, ambiguity; every tile of the view kernel on one shape"""
    for n in TAXA:
        codes, weights = _alignment(n, P, protein, 100 * P + n)
        eng = _engine(codes, weights, protein)
        assert eng.num_informative == P
        wit = pw.PolyWitness(codes, weights, 1 if protein else 0)
        N = int(weights.sum())
        for k, (first, nbr) in enumerate(_shapes(n, n + P)):
            for root in (1, n):
                _check(eng, wit, first, nbr, root, (n, k, root), n_sites=N)
        for tile in POLY_TILES:
            eng.set_option("poly_tile", tile)
            _check(eng, wit, first, nbr, n, (n, "tile", tile))


@pytest.mark.parametrize("sites", SITES)
def test_fitch_at_the_tile_edges(sites):
    """DNA rows of more than one tile, every brlen_tile shape and view tile, with and without 64-bit addressing"""
    from mpboot_amd import trees
    n, P = 16, 257
    codes, weights = _alignment(n, P, False, sites)
    weights = (weights + (sites - int(weights.sum())) // P).astype(np.int32)
    weights[-1] += sites - int(weights.sum())
    assert int(weights.sum()) == sites and weights.min() >= 1
    rng = np.random.default_rng(sites)
    first, nbr = pw.random_collapse(trees.random_topology(n, rng), n, rng, 0.4)
    wit = pw.PolyWitness(codes, weights, 0)
    for big in (0, 1):
        eng = _engine(codes, weights, False)
        eng.set_option("force_big", big)
        for tile in BRLEN_TILES:
            eng.set_option("brlen_tile", tile)
            _check(eng, wit, first, nbr, n, (big, tile), patterns=tile == -1)
        for tile in POLY_TILES:
            eng.set_option("poly_tile", tile)
            _check(eng, wit, first, nbr, 1, (big, "poly", tile))


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_wide_stars(protein, n):
    """a degree beyond a wave's 64 lanes; the resolved tree of as many taxa has more mask rows than one 63-row chunk of the
    per-site counter planes (the star itself has two)"""
    from mpboot_amd import trees
    codes, weights = _alignment(n, 65, protein, n)
    eng = _engine(codes, weights, protein)
    wit = pw.PolyWitness(codes, weights, 1 if protein else 0)
    for root in (1, n):
        _check(eng, wit, *pw.star(n), root, n_sites=int(weights.sum()))
    first, nbr = trees.collapse_branches(trees.random_topology(n, np.random.default_rng(n)), n, ())
    assert len(first) > 63                                  # n - 2 up views + the root edge: more mask rows than one chunk
    _check(eng, wit, first, nbr, 1)


@pytest.mark.parametrize("keep_all", [False, True], ids=["informative", "keep_all"])
@pytest.mark.parametrize("name", ["dna_ambig", "aa", "dna_48"])
def test_fixtures_and_dropped_patterns(name, keep_all):
    """an engine that drops uninformative patterns returns 0 for them and counts the kept ones"""
    from helpers import load_fixture
    from mpboot_amd import engine, trees
    fx = load_fixture(name)
    codes, weights = fx["codes_np"], fx["weights_np"]
    n = codes.shape[0]
    eng = engine.FitchEngine(codes, weights, datatype=fx["datatype"], keep_all=keep_all)
    wit = pw.PolyWitness(codes, weights, fx["datatype"], keep=None if keep_all else fx["informative"])
    rng = np.random.default_rng(2)
    first, nbr = pw.random_collapse(trees.random_topology(n, rng), n, rng, 0.4)
    for root in (1, n):
        _check(eng, wit, first, nbr, root, n_sites=int(weights.sum()))


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_a_resolved_tree_is_the_binary_engine_bit_for_bit(protein):
    from mpboot_amd import trees
    n, P = 40, 129
    codes, weights = _alignment(n, P, protein, 21)
    back = trees.random_topology(n, np.random.default_rng(21))
    first, nbr = trees.collapse_branches(back, n, ())
    for cost in (None, cases.cost_of("asym", 20 if protein else 4)):
        eng = _engine(codes, weights, protein, cost=cost)
        for root in (1, n):
            eng.set_tree(back)
            want_len, want_ptn = _parsimony_at(eng, root)
            a, b, s = eng.branch_substitutions(root)
            _a, _b, ln = eng.branch_lengths(1000, root)
            pa, pb, ps = eng.polytomy_branch_substitutions(first, nbr, root)
            _pa, _pb, pln = eng.polytomy_branch_lengths(first, nbr, 1000, root)
            assert (pa == a).all() and (pb == b).all() and (ps == s).all()
            assert pln.tobytes() == ln.tobytes()
            got_len, got_ptn = eng.polytomy_parsimony(first, nbr, root, with_patterns=True)
            assert got_len == want_len and (got_ptn == want_ptn).all()
        eng.set_tree(back)
        assert eng.polytomy_parsimony(first, nbr, 1) == eng.score_tree(back)


def test_unit_cost_parstree_takes_the_tree_length():
    from mpboot_amd import trees
    n, P = 16, 65
    codes, weights = _alignment(n, P, False, 5)
    rng = np.random.default_rng(5)
    first, nbr = pw.random_collapse(trees.random_topology(n, rng), n, rng, 0.5)
    eng = _engine(codes, weights, False)
    wit = pw.PolyWitness(codes, weights, 0)
    for root in (1, n):
        length = wit.parsimony(first, nbr, root)[0]
        a, b, ln = eng.polytomy_branch_lengths(first, nbr, 8 * length, root, unit_cost_parstree=True)
        assert (_ulps(ln, pw.branch_lengths([length] * len(ln), 8 * length, 4)) <= 4).all()


# ---------------------------------------------------------------- the weighted engine
@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_weighted_equals_the_witness(protein, P):
    """unit costs, a symmetric and a non-symmetric matrix; 16-bit and 32-bit stores"""
    S = 20 if protein else 4
    for i, n in enumerate(TAXA):
        kind = ("unit", "metric", "asym")[(i + COUNTS.index(P)) % 3]
        cost = (1 - np.eye(S, dtype=np.int64)).astype(np.uint32) if kind == "unit" else cases.cost_of(kind, S, seed=7 + i)
        codes, weights = _alignment(n, P, protein, 100 * P + n)
        wit = pw.PolyWitness(codes, weights, 1 if protein else 0, cost=cost)
        eng = _engine(codes, weights, protein, cost=cost)
        assert eng.num_informative == P
        shapes = _shapes(n, n + P)
        for short in (1, 0):
            eng.set_option("sankoff_short", short)
            assert eng.get_option("sankoff_packed") == short
            for k, (first, nbr) in enumerate(shapes if short else shapes[1:4]):
                for root in (1, n):
                    _check(eng, wit, first, nbr, root, (n, kind, short, k, root), n_sites=int(weights.sum()))
            for tile in POLY_TILES:                         # every tile of the view kernel under both store forms
                eng.set_option("poly_tile", tile)
                _check(eng, wit, *shapes[1], n, (n, short, "tile", tile))
            eng.set_option("poly_tile", 0)


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_weighted_wide_star_takes_the_32_bit_store(protein):
    """130 tips under a matrix with large entries: the engine's guard 3 n (max cost + 1) < 2^16 fails, the store is 32-bit, and the sum
    over 129 inputs is exact"""
    n, S = 130, 20 if protein else 4
    cost = (cases.cost_of("asym", S, seed=3).astype(np.int64) * 60).astype(np.uint32)
    assert 3 * n * (int(pw.closed(cost).max()) + 1) >= 65536
    codes, weights = _alignment(n, 65, protein, 9)
    eng = _engine(codes, weights, protein, cost=cost)
    assert eng.get_option("sankoff_packed") == 0
    wit = pw.PolyWitness(codes, weights, 1 if protein else 0, cost=cost)
    for root in (1, n):
        _check(eng, wit, *pw.star(n), root)
    small = cases.cost_of("asym", S, seed=3)                # ... and the stars of 130 and of 65 tips in the 16-bit store
    for m in (n, 65):
        eng = _engine(codes[:m], weights, protein, cost=small)
        assert eng.get_option("sankoff_packed") == 1
        wit = pw.PolyWitness(codes[:m], weights, 1 if protein else 0, cost=small)
        for root in (1, m):
            _check(eng, wit, *pw.star(m), root)
    eng.set_option("sankoff_short", 0)                      # the star of 65 in the 32-bit store
    assert eng.get_option("sankoff_packed") == 0
    _check(eng, wit, *pw.star(65), 1)


def test_weighted_wide_addressing():
    from mpboot_amd import trees
    n, P = 16, 129
    cost = cases.cost_of("asym", 4)
    codes, weights = _alignment(n, P, False, 5)
    rng = np.random.default_rng(2)
    first, nbr = pw.random_collapse(trees.random_topology(n, rng), n, rng, 0.5)
    eng = _engine(codes, weights, False, cost=cost)
    eng.set_option("force_big", 1)
    _check(eng, pw.PolyWitness(codes, weights, 0, cost=cost), first, nbr, 1)


# ---------------------------------------------------------------- statelessness, refusals, size
@pytest.mark.parametrize("weighted", [False, True], ids=["fitch", "weighted"])
def test_the_engines_own_tree_is_untouched(weighted):
    """tree, score, branch substitutions and an SPR scan (the word-major copy) after the calls are what they were before"""
    from mpboot_amd import trees
    n, P = 40, 129
    codes, weights = _alignment(n, P, False, 8)
    back = trees.random_topology(n, np.random.default_rng(8))
    eng = _engine(codes, weights, False, cost=cases.cost_of("asym", 4) if weighted else None)
    eng.set_tree(back)
    score = eng.score_tree(back)
    subst = [x.tolist() for x in eng.branch_substitutions(n)]
    sweep = None if weighted else eng.sweep_scan(1, 3)      # (the planned scan reads the word-major copy)
    rng = np.random.default_rng(9)
    first, nbr = pw.random_collapse(trees.random_topology(n, rng), n, rng, 0.5)
    wit = pw.PolyWitness(codes, weights, 0, cost=cases.cost_of("asym", 4) if weighted else None)
    _check(eng, wit, first, nbr, 1)
    assert (eng.get_tree() == back).all()
    assert [x.tolist() for x in eng.branch_substitutions(n)] == subst
    assert weighted or eng.sweep_scan(1, 3) == sweep
    _check(eng, wit, first, nbr, n)
    assert eng.score_tree(back) == score and (eng.get_tree() == back).all()
    assert eng.optimize_spr(1, 3) <= score


@pytest.mark.parametrize("weighted", [False, True], ids=["fitch", "weighted"])
def test_a_tracker_books_nothing(weighted):
    from mpboot_amd import trees
    n, P = 16, 129
    codes, weights = _alignment(n, P, False, 8)
    back = trees.random_topology(n, np.random.default_rng(8))
    cost = cases.cost_of("metric", 4) if weighted else None
    eng = _engine(codes, weights, False, cost=cost)
    eng.set_tree(back)
    score = eng.score_tree(back)
    samples = np.random.default_rng(5).multinomial(P, np.ones(P) / P, size=4).astype(np.uint16)
    eng.ufboot_attach(samples)
    before = [x.tolist() for x in eng.ufboot_state()]
    rng = np.random.default_rng(3)
    first, nbr = pw.random_collapse(back, n, rng, 0.5)
    _check(eng, pw.PolyWitness(codes, weights, 0, cost=cost), first, nbr, 1)
    assert [x.tolist() for x in eng.ufboot_state()] == before and (eng.get_tree() == back).all()
    assert eng.score_tree(back) == score


def test_no_tree_is_needed_and_malformed_trees_are_refused():
    from mpboot_amd import engine
    codes, weights = _alignment(6, 65, False, 13)
    for n in (5, 6):
        eng = _engine(codes[:n], weights, False)
        wit = pw.PolyWitness(codes[:n], weights, 0)
        _check(eng, wit, *pw.star(n), 1)                    # (no set_tree before)
        if n == 5:
            _check(eng, wit, np.array(pw.GOOD5[0], dtype=np.int32), np.array(pw.GOOD5[1], dtype=np.int32), 5)
        for name, nn, first, nbr in pw.MALFORMED:
            if nn != n:
                continue
            for call in (lambda: eng.polytomy_parsimony(first, nbr if len(nbr) else [0]),
                         lambda: eng.polytomy_branch_substitutions(first, nbr if len(nbr) else [0]) if len(first) > 1 else eng.polytomy_parsimony(first, [0])):
                with pytest.raises(engine.MpfError) as ei:
                    call()
                assert ei.value.code == -2, name            # MPF_E_INVALID
        for root in (0, n + 1):
            with pytest.raises(engine.MpfError):
                eng.polytomy_parsimony(*pw.star(n), root)
        with pytest.raises(engine.MpfError):
            eng.polytomy_branch_lengths(*pw.star(n), 0)
        with pytest.raises(engine.MpfError):
            eng.set_option("poly_tile", 3)
        _check(eng, wit, *pw.star(n), n)                    # ... and served afterwards


def test_at_size():
    """200 x 10 000 DNA, about a third of the inner branches contracted, one tree, both engines"""
    from mpboot_amd import synth, trees
    nt, L = 200, 10000
    letters, _ = synth.synth_alignment(nt, L, "DNA", 0.08, seed=4)
    codes = synth.letters_to_codes(letters, "DNA")
    weights = np.ones(codes.shape[1], dtype=np.int32)
    rng = np.random.default_rng(5)
    first, nbr = pw.random_collapse(trees.random_topology(nt, rng), nt, rng, 1 / 3)
    assert 0.2 * nt < nt - 2 - (len(first) - 1) < 0.45 * nt and int(np.diff(first).max()) > 3
    eng = _engine(codes, weights, False)
    _check(eng, pw.PolyWitness(codes, weights, 0), first, nbr, 1, n_sites=L)
    cost = cases.cost_of("asym", 4)
    _check(_engine(codes, weights, False, cost=cost), pw.PolyWitness(codes, weights, 0, cost=cost), first, nbr, 1)
