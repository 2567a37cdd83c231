"""Taxon insertion on the weighted (-cost) engine (mpf_insertion_costs / mpf_place_taxa / mpf_iq_parsimony_tree under the option
"place_weighted": k_poly_snk_views + k_snk_place_costs + k_place_best) against tests/place_snk_witness.py and against the engine's own
mpf_compute_parsimony_at on the completed tree.  Exact integer equality throughout.

cost(q, b) is the FULL length of the completed tree evaluated at the new taxon's edge.  The witness's from-scratch form (every
completed tree built and scored on its own) checks every entry at n <= 6 and three branches of every query of every backbone and
root at 16 and 40 taxa (there with a table of subtree rows kept from one completed tree to the next); every entry of every case is
compared with the vectorised form, which tests/test_place_snk_witness.py shows equal
to the from-scratch form, to polytomy_witness.recursive_weighted and to oracle/sankoff_slow.py.  The witness does not depend on the
store, so a case's expected matrix is computed once and compared under both stores.

Every engine here sets place_weighted = 1: on an engine without the option this file fails."""
import ctypes as C

import numpy as np
import pytest

import place_snk_witness as psw
import place_witness as plw
from nni_snk_cases import cost_of

pytestmark = pytest.mark.gpu

TAXA = (4, 5, 6, 16, 40)
COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)    # kept patterns: the element-tile edges in both stores
ALPHABETS = ("dna", "aa", "m32")                          # 4, 20 and 32 state rows: everything dispatch_states serves
DT = {"dna": 0, "aa": 1, "m32": 3}
STATES = {"dna": 4, "aa": 20, "m32": 32}
KINDS = {"dna": ("tstv", "metric", "asym"), "aa": ("metric", "asym"), "m32": ("metric", "asym")}
NARROW, WIDE = 1, 2
# k_snk_place_costs' instantiated shapes (host/pair_tile.hpp): (query tile, branch tile, ELEMENTS per K slice; an element is one pattern in the
# 32-bit store and two in the 16-bit store)
SHAPES = {("dna", NARROW): (4, 16, 16), ("aa", NARROW): (4, 16, 16), ("m32", NARROW): (4, 16, 16),
          ("dna", WIDE): (64, 64, 16), ("aa", WIDE): (64, 64, 4), ("m32", WIDE): (32, 32, 4)}


def _alignment(n, P, alphabet, seed):
    """random tip codes with 10 % ambiguity and unknowns, weights 1 .. 5"""
    rng = np.random.default_rng(seed)
    if alphabet == "aa":
        codes, odd = rng.integers(0, 20, size=(n, P)), rng.integers(20, 23, size=(n, P))
    elif alphabet == "m32":
        codes, odd = rng.integers(0, 32, size=(n, P)), np.full((n, P), 32)
    else:
        codes, odd = 1 << rng.integers(0, 4, size=(n, P)), rng.integers(1, 16, size=(n, P))
    codes = np.where(rng.random((n, P)) < 0.1, odd, codes).astype(np.uint8)
    return codes, rng.integers(1, 6, size=P).astype(np.int32)


def _engine(codes, weights, alphabet, cost, keep_all=True, weighted=1):
    from mpboot_amd import engine
    eng = engine.FitchEngine(codes, weights, datatype=DT[alphabet], keep_all=keep_all, cost=cost)
    eng.set_option("place_weighted", weighted)
    assert eng.get_option("place_weighted") == weighted
    return eng


def _store(eng, short):
    eng.set_option("sankoff_short", short)
    assert eng.get_option("sankoff_packed") == short


def _at(eng, back, root):
    """mpf_compute_parsimony_at: every vector made again, the tree evaluated at the leaf root's edge"""
    from mpboot_amd import engine
    s = C.c_uint32()
    back = np.ascontiguousarray(back, dtype=np.int32)
    rc = engine.load_library().mpf_compute_parsimony_at(eng.h, back.ctypes.data_as(C.c_void_p), root, C.byref(s), None)
    assert rc == 0
    return int(s.value)


def _expect(wit, first, nbr, queries, root, rng=None, scratch="all", what=None):
    """the case's expected (branches, matrix, backbone length), checked against the from-scratch form; scratch: 'all' | 'sample' (three
    branches per query; the recursion over each completed tree takes the rows of subtrees it met in an earlier one from a table,
    place_snk_witness.costs(reuse=True), which tests/test_place_snk_witness.py shows to change nothing) | None"""
    br, want, length = wit.view_costs(first, nbr, queries, root)
    assert br == plw.walk(first, nbr, wit.n, root), what
    if scratch == "all":
        assert (wit.costs(first, nbr, queries, root)[1] == want).all(), what
    elif scratch == "sample":
        pick = [set(rng.permutation(len(br))[:3].tolist()) for _ in queries]
        got = wit.costs(first, nbr, queries, root, branches=pick, reuse=True)[1]
        assert all(len(s) == 3 for s in pick)
        assert all(got[q, i] == want[q, i] for q, s in enumerate(pick) for i in s), what
    return br, want, length


def _compare(eng, expect, first, nbr, queries, root, what=None):
    """insertion_costs and place_taxa against an expected (branches, matrix, length)"""
    br, want, length = expect
    a, b, cost, tl = eng.insertion_costs(first, nbr, queries, root)
    assert list(zip(a.tolist(), b.tolist())) == br, what
    assert tl == length and cost.shape == want.shape and (cost.astype(np.int64) == want).all(), what
    at, n1, n2, ln, tl2 = eng.place_taxa(first, nbr, queries, root)
    assert tl2 == length, what
    assert at.tolist() == [plw.first_min(r) for r in want.tolist()] == [int(np.argmin(r)) for r in want], what
    assert list(zip(n1.tolist(), n2.tolist())) == [br[i] for i in at.tolist()], what
    assert ln.tolist() == want.min(axis=1).tolist(), what


def _check(eng, wit, first, nbr, queries, root, rng=None, scratch="all", what=None):
    expect = _expect(wit, first, nbr, queries, root, rng, scratch, what)
    _compare(eng, expect, first, nbr, queries, root, what)
    return expect[0], expect[1]


def _rest(n, tips):
    return [t for t in range(1, n + 1) if t not in [int(x) for x in tips]]


# ---------------------------------------------------------------- costs against the witness
@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_costs_equal_the_witness(alphabet, P):
    """backbones of m = 3 .. n - 1 tips, every absent taxon a query; every root at n <= 6, two roots at 16, one or two at 40; both
    stores.  From scratch: every entry at n <= 6; at 16 and 40 three branches of EVERY query of EVERY backbone and root.  Every
    matrix kind at n <= 16; at 40 taxa the kinds rotate over P (each kind meets 40 taxa at three or more pattern counts and in
    both stores): the witness's share of a 40-taxon case is what bounds the test's time"""
    for i, n in enumerate(TAXA):
        for kind in (KINDS[alphabet] if n <= 16 else (KINDS[alphabet][COUNTS.index(P) % len(KINDS[alphabet])],)):
            _costs_case(alphabet, P, i, n, kind)


def _costs_case(alphabet, P, i, n, kind):
    cost = cost_of(kind, STATES[alphabet], seed=7 + i)
    codes, weights = _alignment(n, P, alphabet, 100 * P + n)
    eng = _engine(codes, weights, alphabet, cost)
    assert eng.num_informative == P and eng.S == STATES[alphabet]
    wit = psw.SnkPlaceWitness(codes, weights, DT[alphabet], cost)
    rng = np.random.default_rng(n + P)
    cases = []
    for m in range(3, n):
        tips = rng.permutation(n)[:m] + 1
        first, nbr = plw.backbone(n, tips, rng)
        rest = _rest(n, tips)
        roots = tips.tolist() if n <= 6 else ([int(tips[0]), int(tips[-1])] if n == 16 or m % 4 == 3 else [int(tips[0])])
        for root in roots:
            scratch = "all" if n <= 6 else "sample"
            cases.append((first, nbr, rest, root, _expect(wit, first, nbr, rest, root, rng, scratch, (n, kind, m, root))))
    for short in (1, 0):
        _store(eng, short)
        for first, nbr, rest, root, expect in cases:
            _compare(eng, expect, first, nbr, rest, root, (n, kind, short, len(rest), root))


# ---------------------------------------------------------------- against the existing kernels
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_entries_equal_compute_parsimony_at_of_the_completed_tree(alphabet):
    """one taxon dropped from a complete tree: entry (q, b) is mpf_compute_parsimony_at(completed tree, root_taxon = q) on the same
    engine; under a matrix that is not symmetric that is not the value at another leaf"""
    from mpboot_amd import trees
    for n, P in ((5, 65), (16, 129)):
        codes, weights = _alignment(n, P, alphabet, n + P)
        for kind in KINDS[alphabet]:
            eng = _engine(codes, weights, alphabet, cost_of(kind, STATES[alphabet]))
            rng = np.random.default_rng(n)
            back = trees.random_topology(n, rng)
            differs = 0
            for short in (1, 0):
                _store(eng, short)
                for t in (int(rng.integers(2, n + 1)), 1):
                    other = 1 if t != 1 else 2
                    first, nbr = trees.drop_tips(back, n, [t])
                    a, b, cost, _ = eng.insertion_costs(first, nbr, [t], other)
                    assert len(a) == 2 * n - 5
                    for i in (range(len(a)) if n == 5 else rng.permutation(len(a))[:6].tolist()):
                        done = trees.lists_to_back(*trees.insert_tip(first, nbr, n, t, int(a[i]), int(b[i])), n)
                        assert int(cost[0, i]) == _at(eng, done, t), (n, kind, short, t, i)
                        differs += int(cost[0, i]) != _at(eng, done, other)
                    assert _at(eng, back, t) in cost[0].tolist()
            assert (differs > 0) == (kind == "asym"), (n, kind)


# ---------------------------------------------------------------- tile edges of k_snk_place_costs
def _stores_and_addressing(eng):
    for short in (1, 0):
        _store(eng, short)
        for big in (0, 1):
            eng.set_option("force_big", big)
            yield short, big


@pytest.mark.parametrize("tile", [NARROW, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_query_tile_edges(alphabet, tile):
    """one below, at, one above the query tile and above two tiles: n = 3 + Q taxa over a three-tip backbone"""
    tq = SHAPES[alphabet, tile][0]
    cost = cost_of("asym", STATES[alphabet])
    for Q in (tq - 1, tq, tq + 1, 2 * tq + 1):
        n = 3 + Q
        codes, weights = _alignment(n, 70, alphabet, Q)
        eng = _engine(codes, weights, alphabet, cost)
        eng.set_option("place_tile", tile)
        rng = np.random.default_rng(Q)
        tips = rng.permutation(n)[:3] + 1
        rest = _rest(n, tips)
        expect = _expect(psw.SnkPlaceWitness(codes, weights, DT[alphabet], cost), [0, 3], tips.tolist(), rest, int(tips[2]), rng, "sample", Q)
        for short, big in _stores_and_addressing(eng):
            launches = eng.get_option("place_launches")
            _compare(eng, expect, [0, 3], tips.tolist(), rest, int(tips[2]), (Q, short, big))
            assert eng.get_option("place_launches") == launches + 2 and eng.get_option("place_tile") == tile


@pytest.mark.parametrize("tile", [NARROW, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_branch_tile_edges(alphabet, tile):
    """branch counts 2 m - 3 (always odd) around the branch tile: the last below it, the first above it, above two tiles"""
    tb = SHAPES[alphabet, tile][1]
    cost = cost_of("metric", STATES[alphabet])
    for B in (tb - 1, tb + 1, 2 * tb + 1):
        m = (B + 3) // 2
        n = m + 5
        codes, weights = _alignment(n, 70, alphabet, B)
        eng = _engine(codes, weights, alphabet, cost)
        eng.set_option("place_tile", tile)
        rng = np.random.default_rng(B)
        tips = rng.permutation(n)[:m] + 1
        first, nbr = plw.backbone(n, tips, rng)
        rest = _rest(n, tips)
        expect = _expect(psw.SnkPlaceWitness(codes, weights, DT[alphabet], cost), first, nbr, rest, int(tips[0]), rng, "sample", B)
        assert len(expect[0]) == B
        for short, big in _stores_and_addressing(eng):
            _compare(eng, expect, first, nbr, rest, int(tips[0]), (B, short, big))


@pytest.mark.parametrize("tile", [NARROW, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_row_length_edges(alphabet, tile):
    """kept patterns one below, at and one above the K slice (KS elements: KS patterns in the 32-bit store, 2 KS in the 16-bit one)
    and the 32-pattern row pitch, and one pitch more"""
    ks = SHAPES[alphabet, tile][2]
    n = 9
    cost = cost_of("asym", STATES[alphabet])
    edges = sorted({e + d for e in (ks, 2 * ks, 32, 64) for d in (-1, 0, 1)})
    for P in edges:
        codes, weights = _alignment(n, P, alphabet, P)
        eng = _engine(codes, weights, alphabet, cost)
        assert eng.num_informative == P
        eng.set_option("place_tile", tile)
        rng = np.random.default_rng(P)
        tips = rng.permutation(n)[:6] + 1
        first, nbr = plw.backbone(n, tips, rng)
        rest = _rest(n, tips)
        expect = _expect(psw.SnkPlaceWitness(codes, weights, DT[alphabet], cost), first, nbr, rest, int(tips[0]), rng, "sample" if P % 32 else None, P)
        for short, big in _stores_and_addressing(eng):
            _compare(eng, expect, first, nbr, rest, int(tips[0]), (P, short, big))


# ---------------------------------------------------------------- where place_tile 0 draws the line
# place_snk_narrow_below (place.hip): the outputs (queries x branches) from which place_tile 0 takes the wide shape, by (alphabet, 16-bit store)
NARROW_BELOW = {("dna", 1): 5 << 16, ("dna", 0): 15 << 14, ("aa", 1): 5 << 16, ("aa", 0): 17 << 14, ("m32", 1): 5 << 16, ("m32", 0): 17 << 14}


@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_place_tile_0_draws_the_line(alphabet):
    """a 400-tip backbone (797 branches) of 812 taxa on a short row: the last query count below the line runs the narrow shape, the
    next one the wide shape (read-only option "place_shape"), and both give the witness's numbers"""
    n, m, P, S = 812, 400, 33, STATES[alphabet]
    B = 2 * m - 3
    if alphabet == "dna":
        cost = cost_of("tstv", 4)
    else:                                                  # entries 1 and 2: the 16-bit store takes 812 taxa (3 n (2 + 1) < 65536)
        cost = (1 + (np.add.outer(np.arange(S), np.arange(S)) % 2)).astype(np.uint32)
        np.fill_diagonal(cost, 0)
    codes, weights = _alignment(n, P, alphabet, 5)
    eng = _engine(codes, weights, alphabet, cost)
    wit = psw.SnkPlaceWitness(codes, weights, DT[alphabet], cost)
    rng = np.random.default_rng(6)
    tips = rng.permutation(n)[:m] + 1
    first, nbr = plw.backbone(n, tips, rng)
    rest = _rest(n, tips)
    br, want, length = _expect(wit, first, nbr, rest, int(tips[0]), rng, "sample", alphabet)
    assert len(br) == B and eng.get_option("place_tile") == 0
    for short in (1, 0):
        _store(eng, short)
        line = NARROW_BELOW[alphabet, short]
        lo = (line - 1) // B
        assert lo * B < line <= (lo + 1) * B and lo + 1 <= len(rest)
        for Q, shape in ((lo, NARROW), (lo + 1, WIDE)):
            _compare(eng, (br, want[:Q], length), first, nbr, rest[:Q], int(tips[0]), (short, Q))
            assert eng.get_option("place_shape") == shape, (short, Q)


# ---------------------------------------------------------------- computeParsimonyTree
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_iq_parsimony_tree(alphabet):
    from mpboot_amd import engine, trees
    from mpboot_amd.rng import Lcg64
    for i, n in enumerate(TAXA):
        kind = KINDS[alphabet][i % len(KINDS[alphabet])]
        cost = cost_of(kind, STATES[alphabet])
        codes, weights = _alignment(n, 90, alphabet, n)
        eng = _engine(codes, weights, alphabet, cost, keep_all=False)
        wit = psw.SnkPlaceWitness(codes, weights, DT[alphabet], cost, keep=eng.informative())
        g = Lcg64(n)
        s0 = int(g.state)
        want_order = plw.shuffle(n, g)
        w_first, w_nbr, w_len = psw.stepwise(wit, want_order, scratch=n <= 6)
        rev = list(range(n, 0, -1))
        w3 = psw.stepwise(wit, rev, scratch=False)
        for short in (1, 0):
            _store(eng, short)
            first, nbr, lengths, order, state = eng.iq_parsimony_tree(tie_state=s0)
            assert order.tolist() == want_order
            assert state == int(g.state) == int(engine.load_library().mpf_tie_state_after(s0, n - 1))
            assert first.tolist() == [int(x) for x in w_first] and nbr.tolist() == w_nbr and lengths.tolist() == w_len, (n, kind, short)
            # the last length is the final tree's length at the last taxon's edge
            assert int(lengths[-1]) == _at(eng, trees.lists_to_back(first, nbr, n), want_order[-1])
            # an order handed in is taken as given
            f2, n2, l2, o2, st2 = eng.iq_parsimony_tree(order=want_order)
            assert st2 is None and o2.tolist() == want_order and f2.tolist() == first.tolist() and n2.tolist() == nbr.tolist()
            assert l2.tolist() == lengths.tolist()
            f3, n3, l3, _, _ = eng.iq_parsimony_tree(order=rev)
            assert n3.tolist() == w3[1] and l3.tolist() == w3[2]


# ---------------------------------------------------------------- statelessness, refusals, the option
def test_the_engines_own_tree_and_a_tracker_are_untouched():
    from mpboot_amd import trees
    n, P = 40, 129
    codes, weights = _alignment(n, P, "dna", 8)
    cost = cost_of("asym", 4)
    back = trees.random_topology(n, np.random.default_rng(8))
    eng = _engine(codes, weights, "dna", cost)
    eng.set_tree(back)
    score = eng.score_tree(back)
    subst = [x.tolist() for x in eng.branch_substitutions(n)]
    samples = np.random.default_rng(5).multinomial(P, np.ones(P) / P, size=4).astype(np.uint16)
    eng.ufboot_attach(samples)
    before = [x.tolist() for x in eng.ufboot_state()]
    tie = eng.tie_state()
    rng = np.random.default_rng(9)
    wit = psw.SnkPlaceWitness(codes, weights, 0, cost)
    first, nbr = trees.drop_tips(trees.random_topology(n, rng), n, [3, 9, 27])
    _check(eng, wit, first, nbr, [3, 9, 27], 1, rng, "sample")
    assert (eng.get_tree() == back).all() and [x.tolist() for x in eng.branch_substitutions(n)] == subst
    eng.iq_parsimony_tree(order=np.arange(1, n + 1))
    assert [x.tolist() for x in eng.ufboot_state()] == before and eng.tie_state() == tie
    assert (eng.get_tree() == back).all() and eng.score_tree(back) == score
    assert [x.tolist() for x in eng.branch_substitutions(n)] == subst


def test_refusals_and_the_option():
    from mpboot_amd import engine
    n = 9
    codes, weights = _alignment(n, 65, "dna", 1)
    cost = cost_of("metric", 4)

    def code_of(call):
        with pytest.raises(engine.MpfError) as ei:
            call()
        return ei.value.code

    # place_weighted 0 (the default): refused as before
    off = engine.FitchEngine(codes, weights, datatype=0, keep_all=True, cost=cost)
    assert off.get_option("place_weighted") == 0
    for eng in (off, _engine(codes, weights, "dna", cost, weighted=0)):
        assert code_of(lambda: eng.insertion_costs(*plw.GOOD, [6])) == -6
        assert code_of(lambda: eng.place_taxa(*plw.GOOD, [6])) == -6
        assert code_of(lambda: eng.iq_parsimony_tree(order=np.arange(1, n + 1))) == -6
    # place_weighted 1: the checks of the hand-over answer as on the Fitch engine
    eng = _engine(codes, weights, "dna", cost)
    wit = psw.SnkPlaceWitness(codes, weights, 0, cost)
    assert code_of(lambda: eng.insertion_costs(*plw.GOOD, [6, 3])) == -2                     # a query present in the backbone
    assert code_of(lambda: eng.place_taxa(*plw.GOOD, [6, 7, 6])) == -2                       # a query listed twice
    assert code_of(lambda: eng.insertion_costs(*plw.GOOD, [10])) == -2
    for name, (first, nbr, root, verdict) in plw.MALFORMED.items():
        want = -6 if verdict == "unsupported" else -2                                         # degree 4: MPF_E_UNSUPPORTED
        assert code_of(lambda: eng.insertion_costs(first, nbr, [9], root)) == want, name
        assert code_of(lambda: eng.place_taxa(first, nbr, [9], root)) == want, name
    assert code_of(lambda: eng.iq_parsimony_tree(order=[1, 2, 3, 4, 5, 6, 7, 8, 8])) == -2
    # no queries: the branches and the backbone's length; the sizing protocol
    a, b, c, tl = eng.insertion_costs(*plw.GOOD, [])
    assert list(zip(a.tolist(), b.tolist())) == plw.walk(*plw.GOOD, n, 1) and c.shape == (0, 7) and tl == wit.length(*plw.GOOD, 1)
    assert [len(x) for x in eng.place_taxa(*plw.GOOD, [])[:4]] == [0, 0, 0, 0]
    assert eng.insertion_costs(*plw.GOOD, [6, 8], cap=6) == (7, tl)
    a, b, c, _ = eng.insertion_costs(*plw.GOOD, [6, 8], cap=9)                               # more room than needed: rows cap apart
    assert (c.astype(np.int64) == wit.view_costs(*plw.GOOD, [6, 8], 1)[1]).all()
    _check(eng, wit, *plw.GOOD, [6, 7, 8, 9], 5)
    # a Fitch engine takes the option and gives the Fitch results unchanged
    fe = engine.FitchEngine(codes, weights, datatype=0, keep_all=True)
    fe.set_option("place_weighted", 1)
    assert fe.get_option("place_weighted") == 1
    a, b, c, tl = fe.insertion_costs(*plw.GOOD, [6, 7, 8, 9], 5)
    br, want, length = plw.PlaceWitness(codes, weights, 0).view_costs(*plw.GOOD, [6, 7, 8, 9], 5)
    assert list(zip(a.tolist(), b.tolist())) == br and tl == length and (c.astype(np.int64) == want).all()


# ---------------------------------------------------------------- size pins
def _size_pin(alphabet, name, n, sites, kind, n_query, seed):
    """the whole matrix against the vectorised witness under every place_tile; from-scratch trees for all branches of two queries and
    one random branch of every other query"""
    from mpboot_amd import synth, trees
    letters, _ = synth.synth_alignment(n, sites, name, 0.08, seed=seed)
    codes = synth.letters_to_codes(letters, name)
    weights = np.ones(codes.shape[1], dtype=np.int32)
    cost = cost_of(kind, STATES[alphabet])
    eng = _engine(codes, weights, alphabet, cost, keep_all=False)
    assert eng.get_option("sankoff_packed") == 1
    wit = psw.SnkPlaceWitness(codes, weights, DT[alphabet], cost, keep=eng.informative())
    rng = np.random.default_rng(seed + 1)
    queries = (rng.permutation(n)[:n_query] + 1).tolist()
    first, nbr = trees.drop_tips(trees.random_topology(n, rng), n, queries)
    root = next(t for t in range(1, n + 1) if t not in queries)
    expect = _expect(wit, first, nbr, queries, root, scratch=None)
    br, want, _ = expect
    nb = 2 * (n - n_query) - 3
    assert len(br) == nb
    for tile in (0, NARROW, WIDE):
        eng.set_option("place_tile", tile)
        _compare(eng, expect, first, nbr, queries, root, tile)
    pick = [set(range(nb)) if q < 2 else {int(rng.integers(nb))} for q in range(n_query)]
    got = wit.costs(first, nbr, queries, root, branches=pick)[1]
    assert all(got[q, i] == want[q, i] for q, s in enumerate(pick) for i in s)


def test_size_pin_200_by_10000_dna():
    """150-tip backbone, 50 queries, tstv"""
    _size_pin("dna", "DNA", 200, 10000, "tstv", 50, 11)


def test_size_pin_60_by_2000_protein():
    """40-tip backbone (77 branches: beyond one branch tile), 20 queries, a 20 x 20 metric"""
    _size_pin("aa", "AA", 60, 2000, "metric", 20, 13)
