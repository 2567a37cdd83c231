"""Robinson-Foulds distances on the engine (mpf_rf_distances on the split pass plus k_rf_columns, k_rf_rows, k_rf_patch, k_rf_shared,
k_rf_pairs, k_rf_finish) against the witness of tests/rf_witness.py: the size of the symmetric difference of trees.splits(a) and
trees.splits(b), as Python frozensets.  Exact integer equality everywhere; nothing is a tolerance."""
import numpy as np
import pytest

import rf_witness as rw
import splits_witness as sw
from helpers import load_fixture
from mpboot_amd import trees

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _eng(n, P=64, seed=1):
    if n not in _ENGINES:
        from mpboot_amd import engine
        rng = np.random.default_rng(seed)
        codes = (1 << rng.integers(0, 4, size=(n, P))).astype(np.uint8)
        _ENGINES[n] = engine.FitchEngine(codes)
    return _ENGINES[n]


@pytest.fixture(scope="module")
def related130():
    """130 related trees on 40 taxa and their witness matrix, computed once"""
    backs = sw.related_trees(40, 130, 21, 3)
    return backs, rw.all_pairs(backs)


@pytest.mark.parametrize("N", (1, 2, 3, 63, 64, 65, 127, 128, 129, 130))
def test_modes_and_tile_edges(related130, N):
    backs, full = related130
    eng = _eng(40)
    got = eng.rf_distances(backs[:N])
    assert got.dtype == np.int32 and got.shape == (N, N)
    assert (got == full[:N, :N]).all()
    assert (got == got.T).all() and (np.diag(got) == 0).all()
    adj = eng.rf_distances(backs[:N], mode="adjacent")
    assert adj.shape == (N - 1,) and adj.tolist() == [int(full[i, i + 1]) for i in range(N - 1)]
    assert eng.get_option("split_overflow") == 0


@pytest.mark.parametrize("N1,N2", ((1, 1), (1, 130), (65, 3), (70, 70)))
def test_two_sets(N1, N2):
    n = 40
    eng = _eng(n)
    base = trees.random_topology(n, np.random.default_rng(8))

    def family(k, seed):
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(k):
            b = base.copy()
            for _ in range(int(rng.integers(0, 4))):
                b = sw.random_spr(b, n, rng)
            out.append(b)
        return out

    a, b = family(N1, 100 + N1), family(N2, 200 + N2)
    for i in range(min(N1, N2, 3)):                      # a few trees present in both sets
        b[(7 * i) % N2] = a[(3 * i) % N1].copy()
    got = eng.rf_distances(a, b)
    assert got.shape == (N1, N2) and (got == rw.two_sets(a, b)).all()
    assert (got == 0).any()
    assert (eng.rf_distances(a, a) == eng.rf_distances(a)).all()


@pytest.mark.parametrize("n,columns", ((4, 1), (34, 31), (35, 32), (36, 33), (67, 64), (68, 65)))
def test_column_word_edges(n, columns):
    """two identical trees share all n - 3 splits: that many columns, exactly"""
    eng = _eng(n)
    a = trees.random_topology(n, np.random.default_rng(n))
    got = eng.rf_distances([a, a])
    assert eng.get_option("rf_columns") == columns == n - 3
    assert got.tolist() == [[0, 0], [0, 0]]
    assert eng.rf_distances([a, a], mode="adjacent").tolist() == [0]
    assert eng.rf_distances([a], [a]).tolist() == [[0]]


def test_quartets_and_mixed_shapes():
    eng = _eng(4)
    names = ["1", "2", "3", "4"]
    q1, q2 = trees.newick_to_back("(1,2,(3,4));", names), trees.newick_to_back("(1,3,(2,4));", names)
    assert rw.rf(q1, q2) == 2
    assert eng.rf_distances([q1, q2]).tolist() == [[0, 2], [2, 0]]
    assert eng.get_option("rf_columns") == 0
    assert eng.rf_distances([q1, q2], mode="adjacent").tolist() == [2]
    assert eng.rf_distances([q1], [q2]).tolist() == [[2]]
    n = 36
    eng = _eng(n)
    a = trees.random_topology(n, np.random.default_rng(n))
    backs = [a, a, sw.caterpillar(n), sw.balanced(n)]
    assert (eng.rf_distances(backs) == rw.all_pairs(backs)).all()
    assert eng.get_option("rf_columns") >= n - 3


@pytest.mark.parametrize("mode", ("all", "adjacent"))
def test_chunks(mode):
    n = 97
    eng = _eng(n)
    backs = sw.related_trees(n, 20, 5, 3)
    want = rw.all_pairs(backs) if mode == "all" else rw.adjacent(backs)
    plain = eng.rf_distances(backs, mode=mode)
    assert eng.get_option("rf_columns") >= 65 and eng.get_option("rf_chunks") == 1
    assert (plain == want).all()
    try:
        for k, least in ((32, 3), (64, 2)):
            eng.set_option("rf_chunk_columns", k)
            got = eng.rf_distances(backs, mode=mode)
            assert eng.get_option("rf_chunks") >= least
            assert eng.get_option("rf_chunks") == -(-eng.get_option("rf_columns") // k)
            assert (got == plain).all()
        eng.set_option("rf_chunk_columns", 33)           # rounded up to 64
        assert (eng.rf_distances(backs, mode=mode) == plain).all()
        assert eng.get_option("rf_chunks") == -(-eng.get_option("rf_columns") // 64)
    finally:
        eng.set_option("rf_chunk_columns", 0)
    assert eng.get_option("rf_chunk_columns") == 0


def test_collisions(related130):
    """4-bit keys: nearly every cluster collides with its slot's representative and the overflow groups carry the columns"""
    backs, full = related130
    backs, full = backs[:40], full[:40, :40]
    eng = _eng(40)
    plain = eng.rf_distances(backs)
    plain_adj = eng.rf_distances(backs, mode="adjacent")
    assert eng.get_option("split_overflow") == 0
    eng.set_option("split_key_bits", 4)
    try:
        masked = eng.rf_distances(backs)
        assert eng.get_option("split_overflow") > 0
        masked_adj = eng.rf_distances(backs, mode="adjacent")
        masked_two = eng.rf_distances(backs[:7], backs[5:])
        eng.set_option("rf_chunk_columns", 32)
        chunked = eng.rf_distances(backs)
        assert eng.get_option("rf_chunks") > 1 and eng.get_option("split_overflow") > 0
    finally:
        eng.set_option("split_key_bits", 64)
        eng.set_option("rf_chunk_columns", 0)
    assert (masked == full).all() and (masked == plain).all() and (chunked == full).all()
    assert (masked_adj == plain_adj).all() and (masked_two == full[:7, 5:]).all()
    assert (eng.rf_distances(backs) == full).all() and eng.get_option("split_overflow") == 0


def test_numbering_and_order_do_not_matter(related130):
    n = 40
    eng = _eng(n)
    names = ["t%d" % i for i in range(1, n + 1)]
    a = trees.random_topology(n, np.random.default_rng(12))
    # the same unrooted tree written from another tip: other inner node numbers, rotated slots
    b = trees.newick_to_back(trees.back_to_newick(a, names, start_tip=17), names)
    assert (a != b).any() and trees.splits(a) == trees.splits(b)
    assert eng.rf_distances([a, b]).tolist() == [[0, 0], [0, 0]]
    assert eng.rf_distances([a], [b]).tolist() == [[0]]
    backs, full = related130
    backs, full = backs[:50], full[:50, :50]
    perm = np.random.default_rng(4).permutation(len(backs))
    got = eng.rf_distances([backs[i] for i in perm])
    assert (got == full[np.ix_(perm, perm)]).all()


def test_refusals():
    from mpboot_amd import engine
    n = 12
    eng = _eng(n)
    rng = np.random.default_rng(2)
    good = [trees.random_topology(n, rng) for _ in range(4)]
    want = rw.all_pairs(good)
    L = engine.load_library()
    flat = np.ascontiguousarray(good, dtype=np.int32)

    def raw(mode, n1, p1, n2, p2, cap):
        out = np.zeros(64, dtype=np.int32)
        return L.mpf_rf_distances(eng.h, mode, n1, p1, n2, p2, cap, out.ctypes.data), out

    def still_serves():
        assert (eng.rf_distances(good) == want).all()

    def refused(call, *words):
        with pytest.raises(engine.MpfError) as err:
            call()
        assert err.value.code == -2                # MPF_E_INVALID
        for w in words:
            assert w in str(err.value)
        still_serves()

    cyc = sw.cyclic_records(good[2], n)
    refused(lambda: eng.rf_distances([good[0], good[1], cyc]), "tree 2", "do not form one tree")
    refused(lambda: eng.rf_distances([good[0], cyc], mode="adjacent"), "tree 1")
    refused(lambda: eng.rf_distances(good, [good[0], cyc, good[1]]), "second set, tree 1")
    refused(lambda: eng.rf_distances([cyc, good[0]], good), "tree 0")
    unlinked = good[1].copy()
    r = int(unlinked[3 * n])
    unlinked[3 * n] = unlinked[r] = -1
    refused(lambda: eng.rf_distances([good[0], unlinked]), "tree 1", "back links")
    refused(lambda: eng.rf_distances(good, [unlinked]), "second set, tree 0")
    p = flat.ctypes.data
    for args in ((engine.RF_ALL_PAIRS, 0, p, 0, None, 64),           # no trees
                 (3, 4, p, 0, None, 64), (-1, 4, p, 0, None, 64),    # an unknown mode
                 (engine.RF_TWO_SETS, 4, p, 0, None, 64),            # two sets without a second set
                 (engine.RF_TWO_SETS, 4, p, 2, None, 64),
                 (engine.RF_ALL_PAIRS, 4, p, 2, p, 64),              # a second set in another mode
                 (engine.RF_ADJACENT, 4, p, 2, p, 64),
                 (engine.RF_ALL_PAIRS, 4, p, 0, None, 15),           # cap one short
                 (engine.RF_ADJACENT, 4, p, 0, None, 2),
                 (engine.RF_TWO_SETS, 4, p, 3, p, 11)):
        rc, _ = raw(*args)
        assert rc == -2, args
        still_serves()
    # cap exact: served
    rc, out = raw(engine.RF_ALL_PAIRS, 4, p, 0, None, 16)
    assert rc == 0 and out[:16].tolist() == want.reshape(-1).tolist()
    rc, out = raw(engine.RF_ADJACENT, 4, p, 0, None, 3)
    assert rc == 0 and out[:3].tolist() == rw.adjacent(good).tolist()
    rc, out = raw(engine.RF_TWO_SETS, 4, p, 3, p, 12)
    assert rc == 0 and out[:12].tolist() == want[:, :3].reshape(-1).tolist()
    # adjacent pairs of one tree: nothing is written, cap 0 will do
    assert L.mpf_rf_distances(eng.h, engine.RF_ADJACENT, 1, p, 0, None, 0, None) == 0


@pytest.fixture(scope="module")
def bb():
    """the small -bb run test_gpu_splits.py uses for ufboot_summarize: (engine with its tracker attached, best tree, n)"""
    from mpboot_amd import engine
    fx = load_fixture("dna_48")
    B = 64
    w0 = fx["weights_np"]
    samples = np.random.default_rng(29).multinomial(int(w0.sum()), w0 / w0.sum(), size=B).astype(np.uint16)
    e = engine.FitchEngine(fx["codes_np"], w0, datatype=fx["datatype"])
    e.seed_ties(engine.TIE_RANDOM, 31)
    e.ufboot_attach(samples)
    e.set_tree(np.array(fx["trees"][2]["back"], dtype=np.int32))
    e.optimize_spr(1, 6)
    return e, e.get_tree(), fx["n"]


def test_no_side_effects(bb):
    e, best, n = bb
    backs = sw.related_trees(n, 9, 3, 3)

    def state():
        return (e.get_tree().tolist(), e.tie_state(), e.ufboot_counters()["tie_draws"], e.ufboot_counters()["events"],
                len(e.ufboot_tree_logl()), [a.tolist() for a in e.ufboot_state()])

    score = e.compute_parsimony()[0]
    before = state()
    assert (e.rf_distances(backs) == rw.all_pairs(backs)).all()
    assert (e.rf_distances(backs, mode="adjacent") == rw.adjacent(backs)).all()
    assert (e.rf_distances(backs, [best]) == rw.two_sets(backs, [best])).all()
    assert state() == before
    assert e.compute_parsimony()[0] == score and (e.get_tree() == best).all()


def test_weighted_engine():
    """the -cost (Sankoff) engine serves the same call"""
    from mpboot_amd import engine
    n = 21
    rng = np.random.default_rng(6)
    codes = (1 << rng.integers(0, 4, size=(n, 64))).astype(np.uint8)
    cost = (np.ones((4, 4), dtype=np.uint32) - np.eye(4, dtype=np.uint32)) * 2
    cost[0, 2] = cost[2, 0] = cost[1, 3] = cost[3, 1] = 1
    e = engine.FitchEngine(codes, cost=cost)
    assert e.weighted
    backs = sw.related_trees(n, 70, 9, 3)
    assert (e.rf_distances(backs) == rw.all_pairs(backs)).all()


def test_size_pin():
    """300 trees x 200 taxa, 0 .. 8 SPR moves each from one tree: 5 x 5 tiles, several words per row"""
    n, N = 200, 300
    backs = sw.related_trees(n, N, 77, 8)
    eng = _eng(n)
    got = eng.rf_distances(backs)
    assert eng.get_option("rf_columns") >= n - 3
    assert (got == rw.all_pairs(backs)).all()


def test_several_k_slices():
    """unrelated trees, each twice: every split of every tree is a column, so a row is longer than one 32-word slice of the
    product kernel, and the slices after the first are the prefetched ones"""
    n = 200
    rng = np.random.default_rng(15)
    distinct = [trees.random_topology(n, rng) for _ in range(12)]
    backs = distinct + [distinct[i] for i in (3, 1, 4, 11, 5, 9, 2, 6, 10, 8, 7, 0)]
    eng = _eng(n)
    want = rw.all_pairs(backs)
    assert (eng.rf_distances(backs) == want).all()
    assert eng.get_option("rf_columns") > 2 * 32 * 32 and eng.get_option("rf_chunks") == 1      # three slices
    assert (eng.rf_distances(backs, mode="adjacent") == rw.adjacent(backs)).all()
    assert (eng.rf_distances(backs[:5], backs[5:]) == want[:5, 5:]).all()


def test_bb_rf(bb):
    from mpboot_amd import bootstrap
    e, best, n = bb
    idx, w, backs = e.ufboot_summary_trees()
    r = bootstrap.bb_rf(e, best)
    want = rw.two_sets(backs, [best])[:, 0]
    assert r["tree_index"].tolist() == idx.tolist() and r["weights"].tolist() == w.tolist()
    assert r["rf"].tolist() == want.tolist()
    assert r["n_distinct_topologies"] == len(set(rw.split_sets(backs)))
    assert r["mean_rf"] == float(sum(int(a) * int(d) for a, d in zip(w, want))) / float(sum(int(a) for a in w))
    assert isinstance(r["mean_rf"], float)
