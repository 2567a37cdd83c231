"""The TBR neighbourhood on the engine (mpf_tbr_scan / mpf_tbr_sweep_best / mpf_apply_tbr / mpf_optimize_tbr on k_tbr_roots +
k_tbr_costs + k_tbr_best) against tests/tbr_witness.py.  Exact integer equality throughout; there is no reference function.

Every matrix is compared with the witness's vectorised form, which tests/test_tbr_witness.py shows equal to its from-scratch form and
to the pinned oracle; the from-scratch form itself checks every entry at n <= 6 and three drawn entries per visit above that.

Tile edges: a list comes in sibling pairs, so 1 + |F| and 1 + |G| are always odd.  Of the values {1, 2, t - 1, t, t + 1} around an
(even) tile edge t only 1, t - 1 and t + 1 can occur; the test asserts that every matrix side it meets is odd and that it covered those.

Size pin: 200 x 10 000 DNA at radius 6."""
import numpy as np
import pytest

import splits_witness as sw
import tbr_witness as tw
from helpers import FIXTURES, load_fixture

pytestmark = pytest.mark.gpu

TAXA = (4, 5, 6, 8, 16, 40)
COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)    # kept patterns: the word, slice and 1024-site row-pitch edges of test_gpu_place.py
ALPHABETS = ("dna", "aa", "m32")
DT = {"dna": 0, "aa": 1, "m32": 3}
RADII = (1, 2, 3, 255)
NARROW, WIDE = 1, 2
# k_tbr_costs' instantiated tiles (place_shape's unweighted rows, host/pair_tile.hpp): (rows of F, columns of G)
SHAPES = {("dna", NARROW): (4, 16), ("aa", NARROW): (4, 16), ("m32", NARROW): (4, 16),
          ("dna", WIDE): (64, 64), ("aa", WIDE): (32, 32), ("m32", WIDE): (32, 32)}


def _engine(codes, weights, alphabet, keep_all=True, cost=None):
    from mpboot_amd import engine
    return engine.FitchEngine(codes, weights, datatype=DT[alphabet], keep_all=keep_all, cost=cost)


def _witness(eng, codes, weights, alphabet, keep_all):
    return tw.TbrWitness(codes, weights, DT[alphabet], keep=None if keep_all else eng.informative())


def _records(n):
    return [3 * t for t in range(1, n + 1)] + [3 * v + s for v in range(n + 1, 2 * n - 1) for s in range(3)]


def _code_of(call):
    from mpboot_amd import engine
    try:
        call()
    except engine.MpfError as err:
        return err.code, str(err)
    return 0, ""


def _scan_equals(eng, wit, back, rec, rad, views, what):
    F, G, want = wit.matrix(back, rec, rad, views)
    f, g, cost = eng.tbr_scan(rec, rad)
    assert f.tolist() == F and g.tolist() == G, what
    assert cost.shape == want.shape and (cost.astype(np.int64) == want).all(), what
    return F, G, want


# ---------------------------------------------------------------- 1. every entry against the witness
@pytest.mark.parametrize("taxa", [TAXA[:5], TAXA[5:]], ids=["n4-16", "n40"])
@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_every_entry_equals_the_witness(alphabet, P, taxa):
    from mpboot_amd import trees
    for n in taxa:
        codes, weights = tw.alignment(n, P, alphabet, 100 * P + n)
        for keep_all in ((True, False) if P >= 63 else (True,)):
            eng = _engine(codes, weights, alphabet, keep_all)
            assert not keep_all or eng.num_informative == P
            wit = _witness(eng, codes, weights, alphabet, keep_all)
            rng = np.random.default_rng(n + P)
            back = trees.random_topology(n, rng)
            length = eng.score_tree(back)
            views = wit.views(back)
            shapes = set()
            for rec in _records(n):
                for rad in RADII:
                    F, G, want = _scan_equals(eng, wit, back, rec, rad, views, (n, keep_all, rec, rad))
                    assert want[0, 0] == length
                    shapes.add(want.shape)
                    fr, gr = [tw.NONE] + F, [tw.NONE] + G
                    if n <= 6:
                        assert (wit.scratch_matrix(back, rec, rad) == want).all(), (n, rec, rad)
                    else:
                        for _ in range(3):
                            i, j = int(rng.integers(len(fr))), int(rng.integers(len(gr)))
                            assert wit.scratch(back, rec, fr[i], gr[j]) == want[i, j], (n, rec, rad, i, j)
            if n == 4:
                assert shapes == {(1, 1), (3, 1), (1, 3)}      # the inner edge, a pendant edge from its tip and from its node
            assert (eng.get_tree() == back).all()


# ---------------------------------------------------------------- 2. pinned where it can be
@pytest.mark.parametrize("name", FIXTURES)
def test_row_0_and_column_0_are_the_spr_scan(name):
    """on every golden fixture: row 0 = spr_scan's p side in order, column 0 at depth >= 2 = its q side, [0][0] = score_tree"""
    fx = load_fixture(name)
    from mpboot_amd import engine
    eng = engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"])
    n = fx["codes_np"].shape[0]
    for sc in fx["scan"]:
        back = np.array(sc["back"], dtype=np.int32)
        assert eng.score_tree(back) == sc["score"]
        rad = sc["maxtrav"]
        for rec in eng.node_order().tolist():
            q, mp, n_p = eng.spr_scan(rec, 1, rad)
            f, g, cost = eng.tbr_scan(rec, rad)
            assert cost[0, 0] == sc["score"]
            assert g.tolist() == q[:n_p].tolist() and cost[0, 1:].tolist() == mp[:n_p].tolist(), (name, rec)
            deep = np.array([i for i, (_r, d) in enumerate(tw.lists(back, n, rec, rad)[0]) if d >= 2], dtype=np.int64)
            assert f[deep].tolist() == q[n_p:].tolist() and cost[1:, 0][deep].tolist() == mp[n_p:].tolist(), (name, rec)


# ---------------------------------------------------------------- 3. tile edges
def _edge_trees():
    from mpboot_amd import trees
    out = [sw.caterpillar(72), sw.caterpillar(80)]
    for n in (72, 80):                                         # balanced: tips joined pairwise, level by level
        first, nbr = [0], []
        nodes, nxt = list(range(1, n + 1)), n + 1
        while len(nodes) > 3:
            up = []
            for a, b in zip(nodes[0::2], nodes[1::2]):
                up.append((nxt, a, b))
                nxt += 1
            rest = [nodes[-1]] if len(nodes) % 2 else []
            nodes = up + rest
        adj = {}

        def link(a, b):
            adj.setdefault(a, []).append(b)
            adj.setdefault(b, []).append(a)

        def lay(x):
            if isinstance(x, tuple):
                link(x[0], lay(x[1]))
                link(x[0], lay(x[2]))
                return x[0]
            return x

        tops = [lay(x) for x in nodes]
        hub = nxt
        for t in tops:
            link(hub, t)
        inner = sorted(v for v in adj if v > n)
        renum = {v: n + 1 + i for i, v in enumerate(inner)}
        for v in inner:
            nbr += [renum.get(u, u) for u in adj[v]]
            first.append(len(nbr))
        out.append(trees.lists_to_back(np.array(first), np.array(nbr), n))
    return out


@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_tile_edges_of_both_shapes(alphabet):
    """caterpillar and balanced trees of 72 and 80 taxa at radius 255, the shape forced both ways and left to the engine"""
    from mpboot_amd import trees
    edges_f = {SHAPES[alphabet, s][0] for s in (NARROW, WIDE)}
    edges_g = {SHAPES[alphabet, s][1] for s in (NARROW, WIDE)}
    want_f = {1} | {t + d for t in edges_f for d in (-1, 1)}
    want_g = {1} | {t + d for t in edges_g for d in (-1, 1)}
    seen_f, seen_g = set(), set()
    for k, back in enumerate(_edge_trees()):
        n = trees.n_taxa_of(back)
        trees.validate(back, n)
        codes, weights = tw.alignment(n, 70, alphabet, 300 + k)
        eng = _engine(codes, weights, alphabet)
        assert eng.S == {"dna": 4, "aa": 20, "m32": 32}[alphabet]
        wit = _witness(eng, codes, weights, alphabet, True)
        eng.score_tree(back)
        views = wit.views(back)
        picked = {}
        for rec in _records(n):
            F, G = tw.lists(back, n, rec, 255)
            rows, cols = 1 + len(F), 1 + len(G)
            assert rows % 2 == 1 and cols % 2 == 1            # (sibling pairs: an even side cannot occur)
            for key in (("f", rows) if rows in want_f - seen_f else None, ("g", cols) if cols in want_g - seen_g else None):
                if key and key not in picked:
                    picked[key] = rec
        for (side, size), rec in picked.items():
            (seen_f if side == "f" else seen_g).add(size)
            for tile in (0, NARROW, WIDE):
                eng.set_option("tbr_tile", tile)
                launches = eng.get_option("tbr_launches")
                _F, _G, want = _scan_equals(eng, wit, back, rec, 255, views, (alphabet, k, rec, tile))
                assert eng.get_option("tbr_launches") == launches + (want.size > 1)
        eng.set_option("tbr_tile", 0)
    assert seen_f == want_f and seen_g == want_g, (sorted(want_f - seen_f), sorted(want_g - seen_g))


# ---------------------------------------------------------------- 4. sweep == scans, whatever the chunking
@pytest.mark.parametrize("alphabet,n,rad", [("dna", 16, 3), ("aa", 16, 255), ("m32", 40, 2), ("dna", 40, 6)])
def test_sweep_equals_the_scans_whatever_the_chunking(alphabet, n, rad):
    from mpboot_amd import trees
    codes, weights = tw.alignment(n, 100, alphabet, 40 + n)
    eng = _engine(codes, weights, alphabet)
    wit = _witness(eng, codes, weights, alphabet, True)
    back = trees.random_topology(n, np.random.default_rng(n + rad))
    eng.score_tree(back)
    order = eng.node_order().tolist()
    assert order == tw.node_order(back, n)
    want, need, cells, mats = [], [], [], []
    for rec in order:
        f, g, cost = eng.tbr_scan(rec, rad)
        best = tw.first_min(cost)
        want.append((tw.NO_BEST, -1, -1) if best is None else (best[0], ([-1] + f.tolist())[best[1]], ([-1] + g.tolist())[best[2]]))
        need.append(len(f) + len(g))
        cells.append(cost.size)
        mats.append(cost)
    assert want == wit.sweep_best(back, rad)[0]
    # the start tip's edge is visited from both ends: the same matrix, transposed
    assert order[0] == 3 and order[n] == int(back[3]) and (mats[0] == mats[n].T).all()
    split = next(cap for cap in range(sum(need), 0, -1) if 3 <= len(tw.chunks(need, cap, cells)) <= 5)
    for cap, chunks in ((0, 1), (1, len(tw.chunks(need, 1, cells))), (split, len(tw.chunks(need, split, cells)))):
        eng.set_option("tbr_chunk_vectors", cap)
        c, f, g, pairs = eng.tbr_sweep_best(rad)
        assert list(zip(c.tolist(), f.tolist(), g.tolist())) == want, cap
        assert pairs == sum(cells) and eng.get_option("tbr_chunks") == chunks, cap
    assert len(tw.chunks(need, 1, cells)) > n


# ---------------------------------------------------------------- 5. stateless
def test_scans_and_sweeps_leave_the_engine_as_it_was():
    from mpboot_amd import engine, trees
    n, P = 24, 150
    codes, weights = tw.alignment(n, P, "dna", 5)
    eng = _engine(codes, weights, "dna")
    back = trees.random_topology(n, np.random.default_rng(5))
    eng.seed_ties(engine.TIE_RANDOM, 17)

    def state():
        return (eng.get_tree().tolist(), eng.score_tree(), [[x.tolist() if hasattr(x, "tolist") else x for x in eng.spr_scan(r, 1, 4)] for r in (3, 3 * n + 3, 3 * (2 * n - 2) + 1)],
                [np.asarray(x).tolist() for x in eng.pattern_scores()], eng.tie_state())

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
    wit = tw.TbrWitness(codes, w2, 0)
    views = wit.views(back)
    for rec in (3, 3 * (n + 2) + 1, 3 * (2 * n - 2)):
        _scan_equals(eng, wit, back, rec, 5, views, rec)
    c, _f, _g, _ = eng.tbr_sweep_best(4)
    assert c.tolist() == [b[0] for b in wit.sweep_best(back, 4)[0]]


# ---------------------------------------------------------------- 6. apply and climb
def test_apply_equals_the_edit_plus_score_tree():
    from mpboot_amd import trees
    n, P = 20, 120
    codes, weights = tw.alignment(n, P, "aa", 8)
    eng, other = _engine(codes, weights, "aa"), _engine(codes, weights, "aa")
    wit = _witness(eng, codes, weights, "aa", True)
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


@pytest.mark.parametrize("rad", (3, 6))
@pytest.mark.parametrize("n", (12, 16, 40))
def test_the_climb_equals_the_witness_move_for_move(n, rad):
    from mpboot_amd import engine, trees
    codes, weights = tw.alignment(n, 300, "dna", n + rad)
    eng = _engine(codes, weights, "dna")
    wit = _witness(eng, codes, weights, "dna", True)
    back = trees.random_topology(n, np.random.default_rng(n * rad))
    eng.seed_ties(engine.TIE_RANDOM, 3)
    tie = eng.tie_state()
    want_back, want_len, want_moves = wit.descent(back, rad)
    assert len(want_moves) >= 3
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
    codes, weights, back = tw.noisy_case(tw.PINNED_SEED)
    eng = _engine(codes, weights, "dna")
    eng.set_tree(back)
    spr = eng.optimize_spr(1, tw.PINNED_RADIUS)
    both, moves = eng.optimize_tbr(tw.PINNED_RADIUS)
    assert both < spr and moves >= 1
    assert both == tw.TbrWitness(codes, weights, 0).length(eng.get_tree())


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_engine_usable():
    from mpboot_amd import trees
    from nni_snk_cases import cost_of
    n, P = 12, 90
    codes, weights = tw.alignment(n, P, "dna", 3)
    back = trees.random_topology(n, np.random.default_rng(3))
    eng = _engine(codes, weights, "dna")
    length = eng.score_tree(back)
    calls = {"scan": lambda e, r: e.tbr_scan(3 * n + 3, r), "sweep": lambda e, r: e.tbr_sweep_best(r),
             "climb": lambda e, r: e.optimize_tbr(r)}
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
    # a tracker attached: nothing would be booked
    samples = np.random.default_rng(5).multinomial(P, np.ones(P) / P, size=4).astype(np.uint16)
    eng.ufboot_attach(samples)
    for name, call in list(calls.items()) + [("apply", lambda e, r: e.apply_tbr(3 * n + 3, -1, -1))]:
        code, msg = _code_of(lambda: call(eng, 3))
        assert code == -6 and "tracker" in msg, name
    eng.ufboot_detach()
    assert eng.tbr_scan(3 * n + 3, 3)[2][0, 0] == length
    # the weighted engine
    snk = _engine(codes, weights, "dna", cost=cost_of("metric", 4))
    snk.score_tree(back)
    for name, call in list(calls.items()) + [("apply", lambda e, r: e.apply_tbr(3 * n + 3, -1, -1))]:
        code, msg = _code_of(lambda: call(snk, 3))
        assert code == -6 and "weighted" in msg, name
    assert snk.score_tree(back) > 0 and (snk.get_tree() == back).all()


# ---------------------------------------------------------------- 8. size pin
def test_size_pin_200_by_10000():
    """radius 6: the sweep's bests on 20 drawn visits plus the five largest matrices against the witness; one move of the climb"""
    from mpboot_amd import synth, trees
    n, sites, rad = 200, 10000, 6
    letters, _ = synth.synth_alignment(n, sites, "DNA", 0.08, seed=11)
    codes = synth.letters_to_codes(letters, "DNA")
    weights = np.ones(codes.shape[1], dtype=np.int32)
    eng = _engine(codes, weights, "dna", keep_all=False)
    wit = _witness(eng, codes, weights, "dna", False)
    back = trees.random_topology(n, np.random.default_rng(2))
    eng.score_tree(back)
    order = eng.node_order().tolist()
    assert order == tw.node_order(back, n)
    c, f, g, pairs = eng.tbr_sweep_best(rad)
    sizes = [(1 + len(F)) * (1 + len(G)) for F, G in (tw.lists(back, n, rec, rad) for rec in order)]
    assert pairs == sum(sizes)
    rng = np.random.default_rng(3)
    at = min(range(len(order)), key=lambda i: (int(c[i]), i))      # the visit the climb will take
    picks = set(np.argsort(sizes)[-5:].tolist()) | set(rng.choice(len(order), size=20, replace=False).tolist()) | {at}
    views = wit.views(back)
    for k in sorted(picks):
        F, G, cost = wit.matrix(back, order[k], rad, views)
        best = tw.first_min(cost)
        assert (int(c[k]), int(f[k]), int(g[k])) == (best[0], ([-1] + F)[best[1]], ([-1] + G)[best[2]]), k
    # one move of the climb: the sweep's lowest cost at its lowest visit
    assert eng.optimize_tbr(rad, 1) == (int(c[at]), 1)
    assert [tuple(int(x) for x in m) for m in zip(*eng.tbr_moves())] == [(order[at], int(f[at]), int(g[at]), int(c[at]))]
    new = trees.apply_tbr(back, order[at], int(f[at]), int(g[at]))
    assert (eng.get_tree() == new).all() and wit.length(new) == int(c[at])
