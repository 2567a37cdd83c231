"""Taxon insertion on the engine (mpf_insertion_costs / mpf_place_taxa / mpf_iq_parsimony_tree on k_poly_views + k_place_costs +
k_place_best) against tests/place_witness.py and the pinned oracle.  Exact integer equality throughout.

The witness's from-scratch form (every tree-plus-taxon built and scored on its own) checks every entry at n <= 6 and, at 16 and 40
taxa, three branches of every query drawn per backbone; every entry of every case is also compared with its vectorised form,
which tests/test_place_witness.py shows equal to the from-scratch form and to the oracle.

Size pin: 200 x 10 000 DNA, 150-tip backbone, 50 queries."""
import numpy as np
import pytest

import place_witness as plw
from helpers import load_fixture

pytestmark = pytest.mark.gpu

TAXA = (4, 5, 6, 16, 40)
COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)    # kept patterns, the row and tile edges of test_gpu_polytomy.py
SITES = (2047, 2048, 2049, 4096, 4097, 8193)              # site totals
ALPHABETS = ("dna", "aa", "m32")
DT = {"dna": 0, "aa": 1, "m32": 3}
NARROW, WIDE = 1, 2
# k_place_costs' instantiated shapes (host/pair_tile.hpp): (query tile, branch tile, words per K slice)
SHAPES = {("dna", NARROW): (4, 16, 16), ("aa", NARROW): (4, 16, 16), ("m32", NARROW): (4, 16, 16),
          ("dna", WIDE): (64, 64, 16), ("aa", WIDE): (32, 32, 4), ("m32", WIDE): (32, 32, 4)}


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


def _engine(codes, weights, alphabet, keep_all=True, cost=None):
    from mpboot_amd import engine
    return engine.FitchEngine(codes, weights, datatype=DT[alphabet], keep_all=keep_all, cost=cost)


def _witness(eng, codes, weights, alphabet, keep_all):
    return plw.PlaceWitness(codes, weights, DT[alphabet], keep=None if keep_all else eng.informative())


def _check(eng, wit, first, nbr, queries, root, rng=None, scratch="all", what=None):
    """insertion_costs and place_taxa against the witness; scratch: 'all' | 'sample' (three branches per query) | None"""
    br, want, length = wit.view_costs(first, nbr, queries, root)
    a, b, cost, tl = eng.insertion_costs(first, nbr, queries, root)
    assert list(zip(a.tolist(), b.tolist())) == br == plw.walk(first, nbr, wit.n, root), what
    assert tl == length and (cost.astype(np.int64) == want).all(), what
    if scratch == "all":
        assert (wit.costs(first, nbr, queries, root)[1] == want).all(), what
    elif scratch == "sample":
        pick = [set(rng.integers(len(br), size=3).tolist()) for _ in queries]
        got = wit.costs(first, nbr, queries, root, branches=pick)[1]
        assert all(got[q, i] == want[q, i] for q, s in enumerate(pick) for i in s), what
    at, n1, n2, ln, tl2 = eng.place_taxa(first, nbr, queries, root)
    assert tl2 == length, what
    assert at.tolist() == [plw.first_min(r) for r in want.tolist()] == [int(np.argmin(r)) for r in want], what
    assert list(zip(n1.tolist(), n2.tolist())) == [br[i] for i in at.tolist()], what
    assert ln.tolist() == want.min(axis=1).tolist(), what
    return br, want


# ---------------------------------------------------------------- costs against the witness
@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_costs_equal_the_witness(alphabet, P):
    """backbones of m = 3 .. n - 1 tips, every absent taxon a query; every root at n <= 6; keep_all on and off"""
    for n in TAXA:
        codes, weights = _alignment(n, P, alphabet, 100 * P + n)
        for keep_all in ((True, False) if P >= 63 else (True,)):
            eng = _engine(codes, weights, alphabet, keep_all)
            assert not keep_all or eng.num_informative == P
            assert alphabet != "m32" or n < 40 or P < 63 or eng.S == 32
            wit = _witness(eng, codes, weights, alphabet, keep_all)
            rng = np.random.default_rng(n + P)
            for m in range(3, n):
                tips = rng.permutation(n)[:m] + 1
                first, nbr = plw.backbone(n, tips, rng)
                rest = [t for t in range(1, n + 1) if t not in tips.tolist()]
                roots = tips.tolist() if n <= 6 else [int(tips[0]), int(tips[-1])]
                for root in roots:
                    _check(eng, wit, first, nbr, rest, root, rng, "all" if n <= 6 else ("sample" if root == roots[0] and m % 6 == 3 else None),
                           (n, m, root, keep_all))


@pytest.mark.parametrize("sites", SITES)
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_costs_at_the_row_edges(alphabet, sites):
    """rows of more than one tile; both shapes of the kernel; with and without 64-bit addressing of the view launch"""
    n, P = 16, 257
    codes, weights = _alignment(n, P, alphabet, sites)
    weights = (weights + (sites - int(weights.sum())) // P).astype(np.int32)
    weights[-1] += sites - int(weights.sum())
    assert int(weights.sum()) == sites and weights.min() >= 1
    rng = np.random.default_rng(sites)
    for big in (0, 1):
        eng = _engine(codes, weights, alphabet)
        eng.set_option("force_big", big)
        wit = _witness(eng, codes, weights, alphabet, True)
        for m in (3, 9, 15):
            tips = rng.permutation(n)[:m] + 1
            first, nbr = plw.backbone(n, tips, rng)
            rest = [t for t in range(1, n + 1) if t not in tips.tolist()]
            for tile in (0, NARROW, WIDE):
                eng.set_option("place_tile", tile)
                _check(eng, wit, first, nbr, rest, int(tips[1]), rng, "sample" if tile == 0 else None, (big, m, tile))


# ---------------------------------------------------------------- tile edges of k_place_costs
@pytest.mark.parametrize("tile", [NARROW, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_query_tile_edges(alphabet, tile):
    """one below, at, one above the query tile and above two tiles: n = 3 + Q taxa over a three-tip backbone"""
    tq = SHAPES[alphabet, tile][0]
    for Q in (tq - 1, tq, tq + 1, 2 * tq + 1):
        n = 3 + Q
        codes, weights = _alignment(n, 70, alphabet, Q)
        eng = _engine(codes, weights, alphabet)
        eng.set_option("place_tile", tile)
        launches = eng.get_option("place_launches")
        rng = np.random.default_rng(Q)
        tips = rng.permutation(n)[:3] + 1
        rest = [t for t in range(1, n + 1) if t not in tips.tolist()]
        _check(eng, _witness(eng, codes, weights, alphabet, True), [0, 3], tips.tolist(), rest, int(tips[2]), rng, "sample", Q)
        assert eng.get_option("place_launches") == launches + 2 and eng.get_option("place_tile") == tile


@pytest.mark.parametrize("tile", [NARROW, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_branch_tile_edges(alphabet, tile):
    """branch counts 2 m - 3 (always odd) around the branch tile: the last below it, the first above it, above two tiles"""
    tb = SHAPES[alphabet, tile][1]
    for B in (tb - 1, tb + 1, 2 * tb + 1):
        m = (B + 3) // 2
        n = m + 5
        codes, weights = _alignment(n, 70, alphabet, B)
        eng = _engine(codes, weights, alphabet)
        eng.set_option("place_tile", tile)
        rng = np.random.default_rng(B)
        tips = rng.permutation(n)[:m] + 1
        first, nbr = plw.backbone(n, tips, rng)
        rest = [t for t in range(1, n + 1) if t not in tips.tolist()]
        br, _ = _check(eng, _witness(eng, codes, weights, alphabet, True), first, nbr, rest, int(tips[0]), rng, "sample", B)
        assert len(br) == B


@pytest.mark.parametrize("tile", [NARROW, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_row_word_edges(alphabet, tile):
    """row words one below, at and one above the K slice (and the 32-word row pitch): unit weights, 32 w - 1, 32 w, 32 w + 1 sites"""
    ks = SHAPES[alphabet, tile][2]
    n = 9
    for w in (ks, 32):
        for P in (32 * w - 1, 32 * w, 32 * w + 1, 32 * (w - 1)):
            codes, _ = _alignment(n, P, alphabet, P)
            weights = np.ones(P, dtype=np.int32)
            eng = _engine(codes, weights, alphabet)
            eng.set_option("place_tile", tile)
            rng = np.random.default_rng(P)
            tips = rng.permutation(n)[:6] + 1
            first, nbr = plw.backbone(n, tips, rng)
            rest = [t for t in range(1, n + 1) if t not in tips.tolist()]
            _check(eng, _witness(eng, codes, weights, alphabet, True), first, nbr, rest, int(tips[0]), rng, "sample" if P % 32 else None, P)


# ---------------------------------------------------------------- pinned lengths
@pytest.mark.parametrize("name", ["dna_ambig", "aa", "bin", "morph32", "dna_dups"])
def test_every_entry_is_the_oracles_length_of_the_completed_tree(name):
    from mpboot_amd import engine, trees
    from oracle import pyoracle as po
    fx = load_fixture(name)
    codes, weights, dt = fx["codes_np"], fx["weights_np"], fx["datatype"]
    n = codes.shape[0]
    rng = np.random.default_rng(len(name))
    back = trees.random_topology(n, rng)
    for keep_all in (False, True):
        eng = engine.FitchEngine(codes, weights, datatype=dt, keep_all=keep_all)
        orc = po.Oracle(codes, weights, datatype=dt, keep_all=keep_all)
        for t in (int(rng.integers(2, n + 1)), 1):
            first, nbr = trees.drop_tips(back, n, [t])
            a, b, cost, tl = eng.insertion_costs(first, nbr, [t], 2 if t == 1 else 1)
            assert len(a) == 2 * n - 5
            for i in range(len(a)):
                done = trees.lists_to_back(*trees.insert_tip(first, nbr, n, t, int(a[i]), int(b[i])), n)
                assert int(cost[0, i]) == orc.score_tree(done), (t, i)
            assert orc.score_tree(back) in cost[0].tolist()


# ---------------------------------------------------------------- the tie rule
def _tie_inputs():
    fx = load_fixture("dna_dups")
    yield "dna_dups", fx["codes_np"], fx["weights_np"]
    for P in (1, 63):
        codes, weights = _alignment(12, P, "dna", 40 + P)
        yield "P%d" % P, codes, weights


def _tied_backbone(wit, n):
    """the first backbone of a fixed search (sizes n - 4, n / 2, 4; seeds 0 .. 19) on which some query's minimum is attained on two
    or more branches; None if there is none"""
    for seed in range(20):
        for m in (n - 4, n // 2, 4):
            rng = np.random.default_rng(seed)
            tips = rng.permutation(n)[:m] + 1
            first, nbr = plw.backbone(n, tips, rng)
            rest = [t for t in range(1, n + 1) if t not in tips.tolist()]
            want = wit.view_costs(first, nbr, rest, int(tips[0]))[1]
            if any((r == r.min()).sum() >= 2 for r in want):
                return first, nbr, rest, tips
    return None


def test_the_first_minimum_in_walk_order():
    differs = 0
    for name, codes, weights in _tie_inputs():
        n = codes.shape[0]
        eng = _engine(codes, weights, "dna")
        wit = plw.PlaceWitness(codes, weights, 0)
        found = _tied_backbone(wit, n)
        assert found is not None, name                                         # a minimum attained on two or more branches
        first, nbr, rest, tips = found
        chosen = []
        for root in tips.tolist():
            br, want = _check(eng, wit, first, nbr, rest, root, None, "all" if root == tips[0] else None, (name, root))
            assert any((r == r.min()).sum() >= 2 for r in want), name
            w_at, w_br, w_len = wit.place(first, nbr, rest, root) if root == tips[0] else (None, None, None)
            at, n1, n2, ln, _ = eng.place_taxa(first, nbr, rest, root)
            assert w_at is None or (at.tolist() == w_at and list(zip(n1.tolist(), n2.tolist())) == w_br and ln.tolist() == w_len), (name, root)
            chosen.append([frozenset(x) for x in zip(n1.tolist(), n2.tolist())])
        differs += sum(x != chosen[0] for x in chosen[1:])
    assert differs > 0                                                         # another root leaf: another walk, another first minimum


# ---------------------------------------------------------------- statelessness, refusals
def test_the_engines_own_tree_and_a_tracker_are_untouched():
    from mpboot_amd import trees
    n, P = 40, 129
    codes, weights = _alignment(n, P, "dna", 8)
    back = trees.random_topology(n, np.random.default_rng(8))
    eng = _engine(codes, weights, "dna")
    eng.set_tree(back)
    score = eng.score_tree(back)
    subst = [x.tolist() for x in eng.branch_substitutions(n)]
    samples = np.random.default_rng(5).multinomial(P, np.ones(P) / P, size=4).astype(np.uint16)
    eng.ufboot_attach(samples)
    before = [x.tolist() for x in eng.ufboot_state()]
    tie = eng.tie_state()
    rng = np.random.default_rng(9)
    wit = plw.PlaceWitness(codes, weights, 0)
    first, nbr = trees.drop_tips(trees.random_topology(n, rng), n, [3, 9, 27])
    _check(eng, wit, first, nbr, [3, 9, 27], 1, rng, "sample")
    assert (eng.get_tree() == back).all() and [x.tolist() for x in eng.branch_substitutions(n)] == subst
    f2, n2, lengths, order, _ = eng.iq_parsimony_tree(order=np.arange(1, n + 1))
    assert [x.tolist() for x in eng.ufboot_state()] == before and eng.tie_state() == tie
    assert (eng.get_tree() == back).all() and eng.score_tree(back) == score
    assert [x.tolist() for x in eng.branch_substitutions(n)] == subst


def test_refusals():
    from mpboot_amd import engine
    n = 9
    codes, weights = _alignment(n, 65, "dna", 1)
    eng = _engine(codes, weights, "dna")
    wit = plw.PlaceWitness(codes, weights, 0)

    def code_of(call):
        with pytest.raises(engine.MpfError) as ei:
            call()
        return ei.value.code

    assert code_of(lambda: eng.insertion_costs(*plw.GOOD, [6, 3])) == -2                     # a query present in the backbone
    assert code_of(lambda: eng.place_taxa(*plw.GOOD, [6, 7, 6])) == -2                       # a query listed twice
    assert code_of(lambda: eng.insertion_costs(*plw.GOOD, [10])) == -2
    for name, (first, nbr, root, verdict) in plw.MALFORMED.items():
        want = -6 if verdict == "unsupported" else -2                                         # degree 4: MPF_E_UNSUPPORTED
        assert code_of(lambda: eng.insertion_costs(first, nbr, [9], root)) == want, name
        assert code_of(lambda: eng.place_taxa(first, nbr, [9], root)) == want, name
    from nni_snk_cases import cost_of
    snk = _engine(codes, weights, "dna", cost=cost_of("metric", 4))
    assert code_of(lambda: snk.insertion_costs(*plw.GOOD, [6])) == -6                        # the weighted engine
    assert code_of(lambda: snk.place_taxa(*plw.GOOD, [6])) == -6
    assert code_of(lambda: snk.iq_parsimony_tree(order=np.arange(1, n + 1))) == -6
    assert code_of(lambda: eng.iq_parsimony_tree(order=[1, 2, 3, 4, 5, 6, 7, 8, 8])) == -2
    with pytest.raises(engine.MpfError):
        eng.set_option("place_tile", 3)
    # no queries: the branches and the backbone's length
    a, b, cost, tl = eng.insertion_costs(*plw.GOOD, [])
    assert list(zip(a.tolist(), b.tolist())) == plw.walk(*plw.GOOD, n, 1) and cost.shape == (0, 7) and tl == wit.length(*plw.GOOD, 1)
    assert [len(x) for x in eng.place_taxa(*plw.GOOD, [])[:4]] == [0, 0, 0, 0]
    # the sizing protocol: too little room fills nothing and reports the count
    assert eng.insertion_costs(*plw.GOOD, [6, 8], cap=6) == (7, tl)
    assert eng.insertion_costs(*plw.GOOD, [6, 8], cap=0) == (7, tl)
    a, b, cost, _ = eng.insertion_costs(*plw.GOOD, [6, 8], cap=9)                            # more room than needed: rows cap apart
    assert (cost.astype(np.int64) == wit.view_costs(*plw.GOOD, [6, 8], 1)[1]).all()
    _check(eng, wit, *plw.GOOD, [6, 7, 8, 9], 5)                                             # ... and served afterwards


def test_one_set_of_lists_three_consumers():
    """the same lists handed to insertion, to the polytomy calls and to a tree set, on one engine that holds a tree: each applies the
    one hand-over check in its own mode"""
    import polytomy_witness as pw
    import split_lists_witness as lw
    from mpboot_amd import engine, trees
    n, P = 9, 65
    codes, weights = _alignment(n, P, "dna", 3)
    eng = _engine(codes, weights, "dna")
    rng = np.random.default_rng(3)
    back = trees.random_topology(n, rng)
    score = eng.score_tree(back)

    def code_of(call):
        with pytest.raises(engine.MpfError) as ei:
            call()
        return ei.value.code

    # a binary backbone with two tips absent: legal for insertion, no tree for the calls that need every tip
    first, nbr = plw.backbone(n, [1, 2, 3, 4, 5, 6, 7], rng)
    _check(eng, plw.PlaceWitness(codes, weights, 0), first, nbr, [8, 9], 1)
    assert code_of(lambda: eng.polytomy_parsimony(first, nbr)) == -2
    assert code_of(lambda: eng.split_counts([back], lists=[(first, nbr)])) == -2
    assert (eng.get_tree() == back).all() and eng.score_tree() == score
    # a backbone with a node of degree 4: a tree for the polytomy calls, unsupported for insertion
    first, nbr = lw.collapse(back, n, 1, rng)
    assert max(np.diff(first)) == 4
    assert code_of(lambda: eng.place_taxa(first, nbr, [9])) == -6
    a, b, subst = eng.polytomy_branch_substitutions(first, nbr)
    br, want = pw.PolyWitness(codes, weights, 0).substitutions(first, nbr)
    assert list(zip(a.tolist(), b.tolist())) == br and (subst.astype(np.int64) == want).all()
    assert (eng.get_tree() == back).all() and eng.score_tree() == score


# ---------------------------------------------------------------- computeParsimonyTree
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_iq_parsimony_tree(alphabet):
    from mpboot_amd import engine, trees
    from mpboot_amd.rng import Lcg64
    from oracle import pyoracle as po
    for n in TAXA:
        codes, weights = _alignment(n, 90, alphabet, n)
        eng = _engine(codes, weights, alphabet, keep_all=False)
        wit = _witness(eng, codes, weights, alphabet, False)
        orc = po.Oracle(codes, weights, datatype=DT[alphabet], keep_all=False)
        g = Lcg64(n)
        s0 = int(g.state)
        want_order = plw.shuffle(n, g)
        first, nbr, lengths, order, state = eng.iq_parsimony_tree(tie_state=s0)
        assert order.tolist() == want_order
        assert state == int(g.state) == int(engine.load_library().mpf_tie_state_after(s0, n - 1))
        w_first, w_nbr, w_len = plw.stepwise(wit, want_order)
        assert first.tolist() == [int(x) for x in w_first] and nbr.tolist() == w_nbr and lengths.tolist() == w_len
        back = trees.lists_to_back(first, nbr, n)
        assert int(lengths[-1]) == orc.score_tree(back)
        eng.set_tree(back)
        assert eng.score_tree(back) == int(lengths[-1])
        # an order handed in is taken as given
        f2, n2, l2, o2, st2 = eng.iq_parsimony_tree(order=want_order)
        assert st2 is None and o2.tolist() == want_order and f2.tolist() == first.tolist() and n2.tolist() == nbr.tolist()
        assert l2.tolist() == lengths.tolist()
        rev = list(range(n, 0, -1))
        f3, n3, l3, _, _ = eng.iq_parsimony_tree(order=rev)
        w3 = plw.stepwise(wit, rev)
        assert n3.tolist() == w3[1] and l3.tolist() == w3[2]


# ---------------------------------------------------------------- size pin
def test_size_pin_200_by_10000():
    """150-tip backbone, 50 queries: the whole matrix against the vectorised witness; from-scratch trees for all branches of two
    queries and one random branch of every other query (the sample covers every query)"""
    from mpboot_amd import synth, trees
    n, sites = 200, 10000
    letters, _ = synth.synth_alignment(n, sites, "DNA", 0.08, seed=11)
    codes = synth.letters_to_codes(letters, "DNA")
    weights = np.ones(codes.shape[1], dtype=np.int32)
    eng = _engine(codes, weights, "dna", keep_all=False)
    wit = _witness(eng, codes, weights, "dna", False)
    rng = np.random.default_rng(12)
    queries = (rng.permutation(n)[:50] + 1).tolist()
    first, nbr = trees.drop_tips(trees.random_topology(n, rng), n, queries)
    root = next(t for t in range(1, n + 1) if t not in queries)
    for tile in (0, NARROW, WIDE):
        eng.set_option("place_tile", tile)
        br, want = _check(eng, wit, first, nbr, queries, root, what=tile, scratch=None)
    assert len(br) == 297
    pick = [set(range(297)) if q < 2 else {int(rng.integers(297))} for q in range(50)]
    got = wit.costs(first, nbr, queries, root, branches=pick)[1]
    assert all(len(s) >= 1 for s in pick)
    assert all(got[q, i] == want[q, i] for q, s in enumerate(pick) for i in s)
