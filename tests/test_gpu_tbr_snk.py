"""The TBR neighbourhood on the weighted (-cost) engine (mpf_tbr_scan / mpf_tbr_sweep_best / mpf_apply_tbr / mpf_optimize_tbr under the
option "tbr_weighted": k_tbr_snk_roots + k_tbr_costs over the min-plus algebra + k_tbr_best) against tests/tbr_snk_witness.py.  Exact
integer equality throughout; there is no reference function.

An entry is the FULL weighted length of the joined tree, cost[0][0] the tree as it is.  Every matrix is compared with the witness's
vectorised form, which tests/test_tbr_snk_witness.py shows equal to its from-scratch form, to oracle/sankoff_slow.py and to
polytomy_witness.recursive_weighted at every root leaf; the from-scratch form itself checks every entry at n <= 6 and three drawn
entries per visit above that.  The witness does not depend on the store, so a case's expected matrices are built once and compared
under both stores (sankoff_short 1 and 0).

Tile edges: a list comes in sibling pairs, so 1 + |F| and 1 + |G| are always odd.  Of the values around an (even) tile edge t only
1, t - 1 and t + 1 can occur; the test asserts that every matrix side it meets is odd and that it covered those.

Every engine here sets tbr_weighted = 1: on an engine without the option this file fails.

Size pin: 200 x 10 000 DNA under tstv at radius 6."""
import numpy as np
import pytest

import tbr_snk_witness as ts
import tbr_witness as tw
from helpers import load_fixture
from nni_snk_cases import cost_of
from test_gpu_tbr import _edge_trees

pytestmark = pytest.mark.gpu

TAXA = (4, 5, 6, 8, 16, 40)
COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)    # kept patterns: the element-tile edges of both stores (test_gpu_place_snk.py)
ALPHABETS = ("dna", "aa", "m32")
DT = {"dna": 0, "aa": 1, "m32": 3}
STATES = {"dna": 4, "aa": 20, "m32": 32}
KINDS = {"dna": ("tstv", "metric"), "aa": ("metric",), "m32": ("metric",)}
RADII = (1, 2, 3, 255)
NARROW, WIDE = 1, 2
# k_tbr_costs' instantiated tiles on the weighted engine (place_shape's weighted rows, host/pair_tile.hpp): (rows of F, columns of G)
SHAPES = {("dna", NARROW): (4, 16), ("aa", NARROW): (4, 16), ("m32", NARROW): (4, 16),
          ("dna", WIDE): (64, 64), ("aa", WIDE): (64, 64), ("m32", WIDE): (32, 32)}


def _engine(codes, weights, alphabet, cost, keep_all=True, weighted=1):
    from mpboot_amd import engine
    eng = engine.FitchEngine(codes, weights, datatype=DT[alphabet], keep_all=keep_all, cost=cost)
    eng.set_option("tbr_weighted", weighted)
    assert eng.get_option("tbr_weighted") == weighted
    return eng


def _store(eng, short):
    eng.set_option("sankoff_short", short)
    assert eng.get_option("sankoff_packed") == short


def _witness(eng, codes, weights, alphabet, cost, keep_all=True):
    return ts.TbrSnkWitness(codes, weights, DT[alphabet], cost, keep=None if keep_all else eng.informative())


def _records(n):
    return [3 * t for t in range(1, n + 1)] + [3 * v + s for v in range(n + 1, 2 * n - 1) for s in range(3)]


def _code_of(call):
    from mpboot_amd import engine
    try:
        call()
    except engine.MpfError as err:
        return err.code, str(err)
    return 0, ""


def _scan_equals(eng, expect, rec, rad, what):
    F, G, want = expect
    f, g, cost = eng.tbr_scan(rec, rad)
    assert f.tolist() == F and g.tolist() == G, what
    assert cost.shape == want.shape and (cost.astype(np.int64) == want).all(), what


# ---------------------------------------------------------------- 1. every entry against the witness
@pytest.mark.parametrize("taxa", [TAXA[:5], TAXA[5:]], ids=["n4-16", "n40"])
@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_every_entry_equals_the_witness(alphabet, P, taxa):
    """every record of the tree, radii 1, 2, 3 and 255 (at 40 taxa 2 and 255), keep_all both ways from 63 patterns up, both stores;
    every matrix kind at n <= 16, at 40 taxa the kinds rotate over P"""
    from mpboot_amd import trees
    for n in taxa:
        kinds = KINDS[alphabet] if n <= 16 else (KINDS[alphabet][COUNTS.index(P) % len(KINDS[alphabet])],)
        radii = RADII if n <= 16 else (2, 255)
        codes, weights = tw.alignment(n, P, alphabet, 100 * P + n)
        for kind in kinds:
            cost = cost_of(kind, STATES[alphabet], seed=7 + n)
            back = trees.random_topology(n, np.random.default_rng(n + P))
            built = {}                                    # kept patterns -> the case's expected matrices (built once per set of patterns)
            for keep_all in ((True, False) if P >= 63 else (True,)):
                eng = _engine(codes, weights, alphabet, cost, keep_all)
                assert eng.S == STATES[alphabet] and (not keep_all or eng.num_informative == P)
                kept = np.ones(P, dtype=bool) if keep_all else np.asarray(eng.informative()) != 0
                if kept.tobytes() not in built:
                    built[kept.tobytes()] = _expected(_witness(eng, codes, weights, alphabet, cost, keep_all), back, n, radii, n + P)
                length, expect = built[kept.tobytes()]
                for short in (1, 0):
                    _store(eng, short)
                    assert eng.score_tree(back) == length
                    for (rec, rad), e in expect.items():
                        _scan_equals(eng, e, rec, rad, (n, kind, keep_all, short, rec, rad))
                    assert (eng.get_tree() == back).all() and eng.score_tree() == length


def _expected(wit, back, n, radii, seed):
    """(length, {(record, radius): (F, G, matrix)}) by the vectorised form, checked against the from-scratch form: every entry at
    n <= 6, three drawn entries per visit above that (memo: the subtree rows kept from one edited tree to the next, which
    tests/test_tbr_snk_witness.py shows to change nothing)"""
    rng = np.random.default_rng(seed)
    length, views = wit.length(back), wit.views(back)
    expect, shapes, memo = {}, set(), {}
    for rec in _records(n):
        for rad in radii:
            F, G, want = expect[rec, rad] = wit.matrix(back, rec, rad, views)
            assert want[0, 0] == length
            shapes.add(want.shape)
            fr, gr = [tw.NONE] + F, [tw.NONE] + G
            if n <= 6:
                assert (wit.scratch_matrix(back, rec, rad) == want).all(), (n, rec, rad)
            else:
                for _ in range(3):
                    i, j = int(rng.integers(len(fr))), int(rng.integers(len(gr)))
                    assert wit.scratch(back, rec, fr[i], gr[j], memo) == want[i, j], (n, rec, rad, i, j)
    if n == 4:
        assert shapes == {(1, 1), (3, 1), (1, 3)}      # the inner edge, a pendant edge from its tip and from its node
    return length, expect


# ---------------------------------------------------------------- 2. pinned where it can be
@pytest.mark.parametrize("name,kind", [("dna_ambig", "tstv"), ("dna_48", "tstv"), ("aa", "metric"), ("aa_40", "metric")])
def test_row_0_and_column_0_are_the_weighted_spr_scan(name, kind):
    """on golden fixtures: row 0 = the weighted spr_scan's p side in order, column 0 at depth >= 2 = its q side, [0][0] = score_tree"""
    fx = load_fixture(name)
    from mpboot_amd import engine
    eng = engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost_of(kind, 20 if fx["datatype"] == 1 else 4))
    eng.set_option("tbr_weighted", 1)
    n = fx["codes_np"].shape[0]
    for short in (1, 0):
        _store(eng, short)
        for sc in fx["scan"]:
            back = np.array(sc["back"], dtype=np.int32)
            length = eng.score_tree(back)
            rad = sc["maxtrav"]
            for rec in eng.node_order().tolist():
                q, mp, n_p = eng.spr_scan(rec, 1, rad)
                f, g, cost = eng.tbr_scan(rec, rad)
                assert cost[0, 0] == length
                assert g.tolist() == q[:n_p].tolist() and cost[0, 1:].tolist() == mp[:n_p].tolist(), (name, rec)
                deep = np.array([i for i, (_r, d) in enumerate(tw.lists(back, n, rec, rad)[0]) if d >= 2], dtype=np.int64)
                assert f[deep].tolist() == q[n_p:].tolist() and cost[1:, 0][deep].tolist() == mp[n_p:].tolist(), (name, rec)


# ---------------------------------------------------------------- 3. tile edges
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_tile_edges_of_both_shapes(alphabet):
    """caterpillar and balanced trees of 72 and 80 taxa at radius 255, the shape forced both ways and left to the engine, both stores"""
    from mpboot_amd import trees
    edges_f = {SHAPES[alphabet, s][0] for s in (NARROW, WIDE)}
    edges_g = {SHAPES[alphabet, s][1] for s in (NARROW, WIDE)}
    want_f = {1} | {t + d for t in edges_f for d in (-1, 1)}
    want_g = {1} | {t + d for t in edges_g for d in (-1, 1)}
    seen_f, seen_g = set(), set()
    cost = cost_of(KINDS[alphabet][0], STATES[alphabet])
    for k, back in enumerate(_edge_trees()):
        n = trees.n_taxa_of(back)
        trees.validate(back, n)
        codes, weights = tw.alignment(n, 70, alphabet, 300 + k)
        eng = _engine(codes, weights, alphabet, cost)
        wit = _witness(eng, codes, weights, alphabet, cost)
        views = wit.views(back)
        picked = {}
        for rec in _records(n):
            F, G = tw.lists(back, n, rec, 255)
            rows, cols = 1 + len(F), 1 + len(G)
            assert rows % 2 == 1 and cols % 2 == 1            # (sibling pairs: an even side cannot occur)
            for key in (("f", rows) if rows in want_f - seen_f else None, ("g", cols) if cols in want_g - seen_g else None):
                if key and key not in picked:
                    picked[key] = rec
        expect = {rec: wit.matrix(back, rec, 255, views) for rec in set(picked.values())}
        for (side, size), rec in picked.items():
            (seen_f if side == "f" else seen_g).add(size)
        for short in (1, 0):
            _store(eng, short)
            eng.score_tree(back)
            for rec, e in expect.items():
                for tile in (0, NARROW, WIDE):
                    eng.set_option("tbr_tile", tile)
                    launches = eng.get_option("tbr_launches")
                    _scan_equals(eng, e, rec, 255, (alphabet, k, short, rec, tile))
                    assert eng.get_option("tbr_launches") == launches + (e[2].size > 1)
            eng.set_option("tbr_tile", 0)
    assert seen_f == want_f and seen_g == want_g, (sorted(want_f - seen_f), sorted(want_g - seen_g))


# ---------------------------------------------------------------- 4. sweep == scans, whatever the chunking
@pytest.mark.parametrize("alphabet,kind,n,rad", [("dna", "tstv", 16, 3), ("aa", "metric", 16, 255), ("m32", "metric", 40, 2), ("dna", "metric", 40, 6)])
def test_sweep_equals_the_scans_whatever_the_chunking(alphabet, kind, n, rad):
    from mpboot_amd import trees
    codes, weights = tw.alignment(n, 100, alphabet, 40 + n)
    cost = cost_of(kind, STATES[alphabet])
    eng = _engine(codes, weights, alphabet, cost)
    wit = _witness(eng, codes, weights, alphabet, cost)
    back = trees.random_topology(n, np.random.default_rng(n + rad))
    want_sweep = wit.sweep_best(back, rad)[0]
    for short in (1, 0):
        _store(eng, short)
        eng.score_tree(back)
        order = eng.node_order().tolist()
        assert order == tw.node_order(back, n)
        want, need, cells, mats = [], [], [], []
        for rec in order:
            f, g, cost_m = eng.tbr_scan(rec, rad)
            best = tw.first_min(cost_m)
            want.append((tw.NO_BEST, -1, -1) if best is None else (best[0], ([-1] + f.tolist())[best[1]], ([-1] + g.tolist())[best[2]]))
            need.append(len(f) + len(g))
            cells.append(cost_m.size)
            mats.append(cost_m)
        assert want == want_sweep
        # the start tip's edge is visited from both ends: the same matrix, transposed (a symmetric cost matrix)
        assert order[0] == 3 and order[n] == int(back[3]) and (mats[0] == mats[n].T).all()
        split = next(cap for cap in range(sum(need), 0, -1) if 3 <= len(tw.chunks(need, cap, cells)) <= 5)
        for cap, chunks in ((0, 1), (1, len(tw.chunks(need, 1, cells))), (split, len(tw.chunks(need, split, cells)))):
            eng.set_option("tbr_chunk_vectors", cap)
            c, f, g, pairs = eng.tbr_sweep_best(rad)
            assert list(zip(c.tolist(), f.tolist(), g.tolist())) == want, (short, cap)
            assert pairs == sum(cells) and eng.get_option("tbr_chunks") == chunks, (short, cap)
        eng.set_option("tbr_chunk_vectors", 0)
        assert len(tw.chunks(need, 1, cells)) > n


# ---------------------------------------------------------------- 5. stateless
def test_scans_and_sweeps_leave_the_engine_as_it_was():
    from mpboot_amd import engine, trees
    n, P = 24, 150
    codes, weights = tw.alignment(n, P, "dna", 5)
    cost = cost_of("tstv", 4)
    eng = _engine(codes, weights, "dna", cost)
    back = trees.random_topology(n, np.random.default_rng(5))
    eng.seed_ties(engine.TIE_RANDOM, 17)

    def state():
        return (eng.get_tree().tolist(), eng.score_tree(), [[x.tolist() if hasattr(x, "tolist") else x for x in eng.spr_scan(r, 1, 4)] for r in (3, 3 * n + 3, 3 * (2 * n - 2) + 1)],
                eng.tie_state())

    for short in (1, 0):
        _store(eng, short)
        eng.set_tree(back)
        before = state()
        for rec in (3, 3 * (n + 2) + 1, 3 * (2 * n - 2)):
            eng.tbr_scan(rec, 5)
        assert state() == before
        eng.tbr_sweep_best(4)
        assert state() == before
    # after set_weights the matrices follow the new weights
    w2 = np.random.default_rng(6).integers(0, 7, size=P).astype(np.int32)
    eng.set_weights(w2)
    eng.set_tree(back)
    wit = ts.TbrSnkWitness(codes, w2, 0, cost)
    views = wit.views(back)
    for rec in (3, 3 * (n + 2) + 1, 3 * (2 * n - 2)):
        _scan_equals(eng, wit.matrix(back, rec, 5, views), rec, 5, rec)
    c, _f, _g, _ = eng.tbr_sweep_best(4)
    assert c.tolist() == [b[0] for b in wit.sweep_best(back, 4)[0]]


# ---------------------------------------------------------------- 6. apply and climb
def test_apply_equals_the_edit_plus_score_tree():
    from mpboot_amd import trees
    n, P = 20, 120
    codes, weights = tw.alignment(n, P, "aa", 8)
    cost = cost_of("metric", 20)
    eng, other = _engine(codes, weights, "aa", cost), _engine(codes, weights, "aa", cost, weighted=0)
    wit = _witness(eng, codes, weights, "aa", cost)
    rng = np.random.default_rng(8)
    back = trees.random_topology(n, rng)
    eng.set_tree(back)
    true_tbr = 0
    for _ in range(50):
        rec = _records(n)[int(rng.integers(4 * n - 6))]
        f, g, _cost = eng.tbr_scan(rec, 255)
        fr, gr = [-1] + f.tolist(), [-1] + g.tolist()
        i, j = int(rng.integers(len(fr))), int(rng.integers(len(gr)))
        true_tbr += i > 0 and j > 0
        new = trees.apply_tbr(back, rec, fr[i], gr[j])
        got = eng.apply_tbr(rec, fr[i], gr[j])
        assert (eng.get_tree() == new).all() and got == other.score_tree(new) == wit.length(new) == _cost[i, j]
        assert eng.node_order().tolist() == other.node_order().tolist() and eng.score_tree() == got
        back = new
    assert true_tbr >= 10


@pytest.mark.parametrize("rad", (2, 255))
@pytest.mark.parametrize("n", (16, 40))
def test_the_climb_equals_the_witness_move_for_move(n, rad):
    from mpboot_amd import engine, trees
    codes, weights = tw.alignment(n, 120 if n == 16 else 60, "dna", n + rad)
    cost = cost_of("tstv", 4)
    eng = _engine(codes, weights, "dna", cost)
    wit = _witness(eng, codes, weights, "dna", cost)
    back = trees.random_topology(n, np.random.default_rng(n * rad))
    eng.seed_ties(engine.TIE_RANDOM, 3)
    tie = eng.tie_state()
    want_back, want_len, want_moves = wit.descent(back, rad)
    assert len(want_moves) >= 3
    for short in (1, 0):
        _store(eng, short)
        eng.set_tree(back)
        assert eng.optimize_tbr(rad, 2) == (want_moves[1][3], 2)
        assert [tuple(int(x) for x in m) for m in zip(*eng.tbr_moves())] == want_moves[:2]
        eng.set_tree(back)
        assert eng.optimize_tbr(rad) == (want_len, len(want_moves))
        assert [tuple(int(x) for x in m) for m in zip(*eng.tbr_moves())] == want_moves
        assert (eng.get_tree() == want_back).all() and eng.tie_state() == tie
        # a local optimum of the whole neighbourhood, the SPR tests among it
        c, _f, _g, _ = eng.tbr_sweep_best(rad)
        assert int(c.min()) >= want_len
        assert int(eng.sweep_costs(1, rad)[1].min()) >= want_len and eng.score_tree() == want_len
        assert eng.optimize_tbr(rad) == (want_len, 0) and len(eng.tbr_moves()[0]) == 0


def test_tbr_goes_on_where_spr_stops_on_the_pinned_seed():
    """the witness's pinned input: from its SPR-local optimum the engine's TBR climb finds the strictly shorter tree the witness finds"""
    codes, weights, back = ts.noisy_case(ts.PINNED_SEED)
    cost = cost_of("tstv", 4)
    wit = ts.TbrSnkWitness(codes, weights, 0, cost)
    spr_back, spr_len, _ = wit.descent(back, ts.PINNED_RADIUS, spr_only=True)
    want_back, want_len, want_moves = wit.descent(spr_back, ts.PINNED_RADIUS)
    eng = _engine(codes, weights, "dna", cost)
    assert eng.score_tree(spr_back) == spr_len and int(eng.sweep_costs(1, ts.PINNED_RADIUS)[1].min()) >= spr_len
    assert eng.optimize_tbr(ts.PINNED_RADIUS) == (want_len, len(want_moves)) and want_len < spr_len
    assert (eng.get_tree() == want_back).all()


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_engine_usable():
    from mpboot_amd import trees
    n, P = 12, 90
    codes, weights = tw.alignment(n, P, "dna", 3)
    back = trees.random_topology(n, np.random.default_rng(3))
    cost = cost_of("metric", 4)
    eng = _engine(codes, weights, "dna", cost)
    length = eng.score_tree(back)
    assert length == ts.TbrSnkWitness(codes, weights, 0, cost).length(back)
    calls = {"scan": lambda e, r: e.tbr_scan(3 * n + 3, r), "sweep": lambda e, r: e.tbr_sweep_best(r),
             "climb": lambda e, r: e.optimize_tbr(r)}
    every = list(calls.items()) + [("apply", lambda e, r: e.apply_tbr(3 * n + 3, -1, -1))]
    for name, call in calls.items():
        for rad in (0, 256, -1):
            code, msg = _code_of(lambda: call(eng, rad))
            assert code == -2 and "maxtrav must be in 1 .. 255" in msg, (name, rad)
    f, g, _ = eng.tbr_scan(3 * n + 3, 255)
    outside_g = next(r for r in _records(n) if r not in g.tolist() and r != -1)
    outside_f = next(r for r in _records(n) if r not in f.tolist())
    for pair in ((-1, outside_g), (outside_f, -1), (f[0] if len(f) else -1, 0), (10 ** 6, -1)):
        code, msg = _code_of(lambda: eng.apply_tbr(3 * n + 3, int(pair[0]), int(pair[1])))
        assert code == -2 and "not in the visit's lists" in msg, pair
    assert _code_of(lambda: eng.tbr_scan(1, 3))[0] == -2 and _code_of(lambda: eng.apply_tbr(10 ** 6, -1, -1))[0] == -2
    assert (eng.get_tree() == back).all() and eng.score_tree() == length
    assert eng.apply_tbr(3 * n + 3, -1, -1) == length and (eng.get_tree() == back).all()      # "none, none": the tree as it is
    # the option off: exactly the refusal of an engine that never had it
    eng.set_option("tbr_weighted", 0)
    for name, call in every:
        code, msg = _code_of(lambda: call(eng, 3))
        assert code == -6 and "weighted" in msg, name
    eng.set_option("tbr_weighted", 1)
    assert eng.tbr_scan(3 * n + 3, 3)[2][0, 0] == length
    # a tracker attached: nothing would be booked
    samples = np.random.default_rng(5).multinomial(P, np.ones(P) / P, size=4).astype(np.uint16)
    eng.ufboot_attach(samples)
    for name, call in every:
        code, msg = _code_of(lambda: call(eng, 3))
        assert code == -6 and "tracker" in msg, name
    eng.ufboot_detach()
    assert eng.tbr_scan(3 * n + 3, 3)[2][0, 0] == length and (eng.get_tree() == back).all()
    # a matrix that is not symmetric: the length depends on the evaluation edge
    asym = _engine(codes, weights, "dna", cost_of("asym", 4))
    at_start = asym.score_tree(back)
    for name, call in every:
        code, msg = _code_of(lambda: call(asym, 3))
        assert code == -6 and "not symmetric" in msg, name
    assert asym.score_tree(back) == at_start and (asym.get_tree() == back).all()
    # a Fitch engine takes the option and ignores it
    from mpboot_amd import engine
    fe = engine.FitchEngine(codes, weights, datatype=0, keep_all=True)
    fe.score_tree(back)
    before = fe.tbr_scan(3 * n + 3, 3)[2]
    fe.set_option("tbr_weighted", 1)
    assert fe.get_option("tbr_weighted") == 1 and (fe.tbr_scan(3 * n + 3, 3)[2] == before).all()
    assert (before == tw.TbrWitness(codes, weights, 0).matrix(back, 3 * n + 3, 3)[2]).all()


# ---------------------------------------------------------------- 8. size pin
def test_size_pin_200_by_10000():
    """radius 6: the sweep's bests on 20 drawn visits plus the five largest matrices against the witness; one move of the climb"""
    from mpboot_amd import synth, trees
    n, sites, rad = 200, 10000, 6
    letters, _ = synth.synth_alignment(n, sites, "DNA", 0.08, seed=11)
    codes = synth.letters_to_codes(letters, "DNA")
    weights = np.ones(codes.shape[1], dtype=np.int32)
    cost = cost_of("tstv", 4)
    eng = _engine(codes, weights, "dna", cost, keep_all=False)
    wit = _witness(eng, codes, weights, "dna", cost, keep_all=False)
    back = trees.random_topology(n, np.random.default_rng(2))
    order = tw.node_order(back, n)
    sizes = [(1 + len(F)) * (1 + len(G)) for F, G in (tw.lists(back, n, rec, rad) for rec in order)]
    rng = np.random.default_rng(3)
    picks = set(np.argsort(sizes)[-5:].tolist()) | set(rng.choice(len(order), size=20, replace=False).tolist())
    views = wit.views(back)
    want = {}
    for k in sorted(picks):
        F, G, m = wit.matrix(back, order[k], rad, views)
        best = tw.first_min(m)
        want[k] = (best[0], ([-1] + F)[best[1]], ([-1] + G)[best[2]])
    for short in (1, 0):
        _store(eng, short)
        eng.score_tree(back)
        assert eng.node_order().tolist() == order
        c, f, g, pairs = eng.tbr_sweep_best(rad)
        assert pairs == sum(sizes)
        for k, w in want.items():
            assert (int(c[k]), int(f[k]), int(g[k])) == w, (short, k)
        # one move of the climb: the sweep's lowest cost at its lowest visit
        at = min(range(len(order)), key=lambda i: (int(c[i]), i))
        assert eng.optimize_tbr(rad, 1) == (int(c[at]), 1)
        assert [tuple(int(x) for x in m) for m in zip(*eng.tbr_moves())] == [(order[at], int(f[at]), int(g[at]), int(c[at]))]
        new = trees.apply_tbr(back, order[at], int(f[at]), int(g[at]))
        assert (eng.get_tree() == new).all() and wit.length(new) == int(c[at])
