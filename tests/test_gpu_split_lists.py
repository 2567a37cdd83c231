"""The split products on trees with polytomies (mpf_split_counts_set, mpf_split_support_set, mpf_consensus_tree_set,
mpf_rf_distances_set; k_split_keys_lists beside k_split_keys, dead cluster slots, per-tree split counts in k_rf_finish) against the
witness of tests/split_lists_witness.py: Python frozensets from splits_witness.list_splits / trees.splits, RF = the size of the
symmetric difference.  Second witness: the host-only program.  Exact integer equality everywhere; nothing is a tolerance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import split_lists_witness as lw
import splits_witness as sw
from helpers import ROOT, load_fixture
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


def _args(items):
    """(backs, lists, the items in the engine's set order: records first, then lists)"""
    backs, lists, perm = lw.as_engine_args(list(items))
    return backs, lists, [items[i] for i in perm]


def _rf(eng, items, items2=None, mode="all"):
    b, l, so = _args(items)
    if items2 is None:
        return eng.rf_distances(b, None, mode, lists=l if l is not None else []), so
    b2, l2, so2 = _args(items2)
    return eng.rf_distances(b, b2, mode, lists=l if l is not None else [], lists2=l2), so, so2


def _check_products(eng, items, weights, n, thresholds=(0.0, 0.5)):
    """counts, consensus and supports (on a contracted target) of a weighted mixed set against the witness"""
    b, l, so = _args(items)
    perm = lw.as_engine_args(list(items))[2]
    w = [int(weights[i]) for i in perm]
    sets = lw.split_sets(so, n)
    words, cnt, total = lw.ordered_table(sets, w, n)
    bits, count, tot = eng.split_counts(b, w, lists=l)
    assert tot == total and count.tolist() == cnt and [tuple(int(x) for x in r) for r in bits] == words
    assert eng.split_counts(b, w, counts_only=True, lists=l) == (len(cnt), total)
    for thr in thresholds:
        (first, nbr, sup), _ = lw.consensus(sets, w, thr, n)
        gf, gn, gs, gt = eng.consensus_tree(b, w, thr, lists=l)
        assert (gf.tolist(), gn.tolist(), gs.tolist(), gt) == (first, nbr, sup, total)
    for target in [t for t in so if lw.is_lists(t)][:3]:
        a, c, s, gt = eng.split_support(b, None, w, lists=l, target_lists=target)
        assert list(zip(a.tolist(), c.tolist(), s.tolist())) == lw.supports(sets, w, target, n) and gt == total
        assert len(a) == n + len(target[0]) - 2


# ---------------------------------------------------------------- fully resolved lists are their record form
@pytest.mark.parametrize("n", (4, 5, 33, 130))
def test_fully_resolved_lists_equal_the_record_calls(n):
    eng = _eng(n)
    backs = sw.related_trees(n, 7, 40 + n, 3)
    lists = [trees.back_to_lists(b, n) for b in backs]
    assert all((trees.lists_to_back(f, x, n) == b).all() for (f, x), b in zip(lists, backs))
    w = [2, 0, 1, 5, 1, 3, 1]
    for ww in (None, w):
        rb, rc, rt = eng.split_counts(backs, ww)
        for kw in (dict(backs=None, lists=lists), dict(backs=backs[:3], lists=lists[3:])):
            gb, gc, gt = eng.split_counts(kw["backs"], ww, lists=kw["lists"])
            assert (gb == rb).all() and (gc == rc).all() and gt == rt
        for thr in (0.0, 0.5):
            want = eng.consensus_tree(backs, ww, thr)
            got = eng.consensus_tree(None, ww, thr, lists=lists)
            assert all(np.array_equal(x, y) for x, y in zip(want[:3], got[:3])) and want[3] == got[3]
        want = eng.split_support(backs, backs[2], ww)
        got = eng.split_support(backs[:2], None, ww, lists=lists[2:], target_lists=lists[2])
        assert all(np.array_equal(x, y) for x, y in zip(want[:3], got[:3])) and want[3] == got[3]
    full = eng.rf_distances(backs)
    cols = eng.get_option("rf_columns")
    assert (eng.rf_distances(None, lists=lists) == full).all() and eng.get_option("rf_columns") == cols
    assert (eng.rf_distances(backs[:4], lists=lists[4:]) == full).all()
    assert (eng.rf_distances(None, mode="adjacent", lists=lists) == eng.rf_distances(backs, mode="adjacent")).all()
    assert (eng.rf_distances(backs[:3], None, lists2=lists[2:]) == full[:3, 2:]).all()
    assert (eng.rf_distances(None, None, lists=lists[:3], lists2=lists[2:]) == full[:3, 2:]).all()


# ---------------------------------------------------------------- mixed sets, all modes, tile edges
@pytest.fixture(scope="module")
def family130():
    """130 related trees on 40 taxa, a random half contracted by 1 .. n - 3 branches, a star and a record tree among the first two"""
    return lw.mixed_family(40, 130, 21, 3)


@pytest.mark.parametrize("N", (2, 63, 64, 65))
def test_mixed_sets_all_pairs_and_adjacent(family130, N):
    n, items = 40, family130[:N]
    eng = _eng(n)
    got, so = _rf(eng, items)
    sets = lw.split_sets(so, n)
    assert sum(1 for t in so if lw.is_lists(t)) >= 1 and not lw.is_lists(so[0]) and any(len(s) == 0 for s in sets)
    assert got.dtype == np.int32 and (got == lw.all_pairs(sets)).all()
    assert (got == got.T).all() and (np.diag(got) == 0).all()
    adj, _ = _rf(eng, items, mode="adjacent")
    assert adj.tolist() == lw.adjacent(sets).tolist()
    assert eng.get_option("split_overflow") == 0


@pytest.mark.parametrize("N1,N2", ((65, 3), (63, 66), (2, 64)))
def test_mixed_two_sets(family130, N1, N2):
    """set sizes on both sides of a tile edge; a record-format tree and a star in each of the two sets"""
    n = 40
    eng = _eng(n)
    a = family130[:N1]                                   # begins with a record tree and the star
    b = [sw.balanced(n), lw.star(n)] + family130[130 - (N2 - 2):] if N2 > 2 else [lw.star(n), sw.caterpillar(n), family130[129]]
    assert len(a) == N1 and len(b) == N2
    got, sa, sb = _rf(eng, a, b)
    for so in (sa, sb):
        assert not lw.is_lists(so[0]) and any(lw.is_lists(t) and len(t[0]) == 2 for t in so)
    want = lw.two_sets(lw.split_sets(sa, n), lw.split_sets(sb, n))
    assert got.shape == (N1, N2) and (got == want).all()
    if N1 == 2:                                          # the star's row: every tree's own number of splits
        assert got[1].tolist() == [len(x) for x in lw.split_sets(sb, n)]


@pytest.mark.parametrize("n", (32, 33, 64, 65))
def test_word_edges(n):
    eng = _eng(n)
    items = lw.mixed_family(n, 9, 300 + n, 3) + [lw.middle_hub(n)]
    got, so = _rf(eng, items)
    assert (got == lw.all_pairs(lw.split_sets(so, n))).all()
    _check_products(eng, items, [1, 2, 0, 3, 1, 1, 4, 1, 2, 1], n)


def test_four_taxa():
    """the smallest engine (mpf_engine_create needs four taxa; three taxa, where every distance is 0, are covered on the host-only
    program in test_split_lists_host.py)"""
    eng = _eng(4)
    names = ["1", "2", "3", "4"]
    q1, q2 = trees.newick_to_back("(1,2,(3,4));", names), trees.newick_to_back("(1,3,(2,4));", names)
    items = [q1, q2, lw.star(4), trees.back_to_lists(q1, 4)]
    got, so = _rf(eng, items)
    assert got.tolist() == [[0, 2, 1, 0], [2, 0, 1, 2], [1, 1, 0, 1], [0, 2, 1, 0]]
    _check_products(eng, items, [1, 1, 3, 1], 4)


# ---------------------------------------------------------------- products
def test_weighted_products(family130):
    n, items = 40, family130[:24]
    w = [(5 * i + 2) % 7 for i in range(len(items))]
    w[1], w[3], w[0] = 6, 0, 0                           # the star counts in the total and holds no split; two trees are left out
    _check_products(_eng(n), items, w, n)


@pytest.mark.parametrize("thr", (0.0, 0.5, 0.9))
def test_consensus_round_trip(family130, thr):
    n = 40
    eng = _eng(n)
    backs = [t for t in family130 if not lw.is_lists(t)][:30]
    w = [1 + i % 3 for i in range(len(backs))]
    first, nbr, sup, total = eng.consensus_tree(backs, w, thr)
    a, c, s, tot = eng.split_support(backs, None, w, target_lists=(first, nbr))
    assert tot == total and len(a) == n + len(first) - 2
    for x, y, z in zip(a.tolist(), c.tolist(), s.tolist()):
        assert z == (-1 if y <= n else int(sup[y - n - 1]))
    # in step with the branch walk of the polytomy calls
    pa, pc, _ = eng.polytomy_branch_substitutions(first, nbr)
    assert (pa == a).all() and (pc == c).all()
    got = eng.rf_distances(backs, None, lists2=[(first, nbr)])[:, 0]
    cons = lw.splits_of((first, nbr), n)
    assert got.tolist() == [len(cons ^ x) for x in lw.split_sets(backs, n)]


def test_collisions(family130):
    """4-bit keys: nearly every cluster collides with its slot's representative; the overflow list carries the result, and a dead
    slot never reaches it"""
    n, items = 40, family130[:40]
    eng = _eng(n)
    plain, so = _rf(eng, items)
    assert eng.get_option("split_overflow") == 0
    sets = lw.split_sets(so, n)
    live = sum(len(s) for s in sets)
    eng.set_option("split_key_bits", 4)
    try:
        masked, _ = _rf(eng, items)
        ovf = eng.get_option("split_overflow")
        assert 0 < ovf < live                            # (with a dead slot on the list it could exceed the live clusters)
        masked_adj, _ = _rf(eng, items, mode="adjacent")
        masked_two, sa, sb = _rf(eng, items[:7], items[5:])
        _check_products(eng, items, [(3 * i + 1) % 4 for i in range(len(items))], n)
        assert eng.get_option("split_overflow") > 0
    finally:
        eng.set_option("split_key_bits", 64)
    assert (masked == plain).all() and (plain == lw.all_pairs(sets)).all()
    assert masked_adj.tolist() == lw.adjacent(sets).tolist()
    assert (masked_two == lw.two_sets(lw.split_sets(sa, n), lw.split_sets(sb, n))).all()


def test_chunks():
    n = 97
    eng = _eng(n)
    items = lw.mixed_family(n, 20, 5, 3)
    plain, so = _rf(eng, items)
    assert (plain == lw.all_pairs(lw.split_sets(so, n))).all() and eng.get_option("rf_chunks") == 1
    eng.set_option("rf_chunk_columns", 32)
    try:
        got, _ = _rf(eng, items)
        assert eng.get_option("rf_chunks") == -(-eng.get_option("rf_columns") // 32) >= 2
        adj, _ = _rf(eng, items, mode="adjacent")
    finally:
        eng.set_option("rf_chunk_columns", 0)
    assert (got == plain).all() and adj.tolist() == [int(plain[i, i + 1]) for i in range(len(items) - 1)]


# ---------------------------------------------------------------- the record calls, the engine's state
def test_records_only_calls_are_unchanged(family130):
    import rf_witness as rw
    n = 40
    eng = _eng(n)
    backs = [t for t in family130 if not lw.is_lists(t)][:20]
    lists = [t for t in family130 if lw.is_lists(t)][:5]

    def record_calls():
        l0 = eng.get_option("split_launches")
        rf = eng.rf_distances(backs)
        opts = {k: eng.get_option(k) for k in ("rf_launches", "rf_columns", "rf_chunks", "split_overflow")}
        assert eng.get_option("split_launches") == l0 + 1
        cnt = eng.split_counts(backs)
        sup = eng.split_support(backs, backs[3])
        con = eng.consensus_tree(backs, None, 0.5)
        opts["split_passes"] = eng.get_option("split_launches") - l0
        return rf, opts, cnt, sup, con

    before = record_calls()
    assert (before[0] == rw.all_pairs(backs)).all() and before[1]["rf_launches"] == 8      # 5 of the pass, rows, product, finish
    eng.rf_distances(backs, None, lists=lists)
    assert eng.get_option("rf_launches") == 9            # one more: the list walk
    eng.split_counts(backs, lists=lists)
    eng.consensus_tree(backs, lists=lists)
    # the set calls on records alone launch what the record calls launch
    assert (eng.rf_distances(backs, None, lists=[]) == before[0]).all()
    assert {k: eng.get_option(k) for k in before[1] if k != "split_passes"} == {k: v for k, v in before[1].items() if k != "split_passes"}
    after = record_calls()
    assert (after[0] == before[0]).all() and after[1] == before[1]
    for x, y in zip(before[2:], after[2:]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    words, cnt, total = lw.ordered_table(lw.split_sets(backs, n), None, n)
    assert after[2][1].tolist() == cnt and after[2][2] == total


@pytest.fixture(scope="module")
def bb():
    """the small -bb run test_gpu_rf.py uses: (engine with its tracker attached, best tree, n)"""
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
    items = lw.mixed_family(n, 9, 3, 3)

    def state():
        return (e.get_tree().tolist(), e.tie_state(), e.ufboot_counters()["tie_draws"], e.ufboot_counters()["events"],
                len(e.ufboot_tree_logl()), [a.tolist() for a in e.ufboot_state()])

    score = e.compute_parsimony()[0]
    before = state()
    got, so = _rf(e, items)
    assert (got == lw.all_pairs(lw.split_sets(so, n))).all()
    _rf(e, items, mode="adjacent")
    _rf(e, items, [best])
    _check_products(e, items, [1] * len(items), n)
    assert state() == before
    assert e.compute_parsimony()[0] == score and (e.get_tree() == best).all()


def test_bb_rf_with_the_consensus(bb):
    from mpboot_amd import bootstrap
    e, best, n = bb
    idx, w, backs = e.ufboot_summary_trees()
    plain = bootstrap.bb_rf(e, best)
    r = bootstrap.bb_rf(e, best, consensus=True)
    assert set(plain) == {"tree_index", "weights", "rf", "mean_rf", "n_distinct_topologies"}
    for k in plain:
        assert np.array_equal(r[k], plain[k])
    sets = lw.split_sets(list(backs), n)
    (first, nbr, sup), total = lw.consensus(sets, w, 0.0, n)
    assert [x.tolist() for x in r["consensus"]] == [first, nbr, sup]
    cons = lw.splits_of((np.array(first), np.array(nbr)), n)
    want = [len(cons ^ s) for s in sets]
    assert r["rf_consensus"].tolist() == want and r["best_rf_consensus"] == len(cons ^ lw.splits_of(best, n))
    assert r["mean_rf_consensus"] == float(sum(int(a) * int(d) for a, d in zip(w, want))) / float(total)


def test_weighted_engine():
    """the -cost (Sankoff) engine serves the same calls"""
    from mpboot_amd import engine
    n = 21
    rng = np.random.default_rng(6)
    codes = (1 << rng.integers(0, 4, size=(n, 64))).astype(np.uint8)
    cost = (np.ones((4, 4), dtype=np.uint32) - np.eye(4, dtype=np.uint32)) * 2
    cost[0, 2] = cost[2, 0] = cost[1, 3] = cost[3, 1] = 1
    e = engine.FitchEngine(codes, cost=cost)
    assert e.weighted
    items = lw.mixed_family(n, 70, 9, 3)
    got, so = _rf(e, items)
    assert (got == lw.all_pairs(lw.split_sets(so, n))).all()
    _check_products(e, items[:12], [1, 2, 0, 1, 1, 3, 1, 1, 2, 1, 1, 1], n)


# ---------------------------------------------------------------- refusals
def test_refusals():
    import ctypes as C

    from mpboot_amd import engine
    n = 9
    eng = _eng(n)
    good = lw.broken_lists("good")
    rec = sw.related_trees(n, 3, 2, 2)
    want, _ = _rf(eng, rec + [good])

    def still_serves():
        assert (eng.rf_distances(rec, lists=[good]) == want).all()

    def refused(call, *words):
        with pytest.raises(engine.MpfError) as err:
            call()
        assert err.value.code == -2                # MPF_E_INVALID
        for w in words:
            assert w in str(err.value), str(err.value)
        still_serves()

    for kind in lw.BROKEN:
        bad = lw.broken_lists(kind)
        refused(lambda: eng.rf_distances(rec, lists=[good, bad]), "list tree 1")
        refused(lambda: eng.rf_distances(rec, None, lists2=[good, good, bad]), "second set, list tree 2")
        refused(lambda: eng.split_counts(rec, lists=[bad, good]), "list tree 0")
        refused(lambda: eng.consensus_tree(None, lists=[good, bad]), "list tree 1")
        refused(lambda: eng.split_support(rec, None, lists=[good], target_lists=bad), "target tree")
    refused(lambda: eng.rf_distances(rec, lists=[good, (np.zeros(9, dtype=np.int32), np.zeros(0, dtype=np.int32))]), "list tree 1")
    refused(lambda: eng.split_counts(rec, [1, 1, 1, -1], lists=[good]), "list tree 0", "negative weight")
    refused(lambda: eng.split_counts(rec, [1, -2, 1, 1], lists=[good]), "tree 1", "negative weight")
    cyc = sw.cyclic_records(rec[1], n)
    refused(lambda: eng.rf_distances([rec[0], cyc], lists=[good]), "tree 1", "do not form one tree")
    # the raw calls: an empty set, a short cap, a second set in a one-set mode
    L = engine.load_library()
    s1, T, _, keep1 = eng._mixed_set(rec, [good])
    s2, _, _, keep2 = eng._mixed_set(None, [good])
    empty = engine.TreeSet()
    out = np.zeros(64, dtype=np.int32)
    p = out.ctypes.data
    assert T == 4
    for args in ((engine.RF_ALL_PAIRS, C.byref(empty), None, 64, p), (engine.RF_ALL_PAIRS, None, None, 64, p),
                 (engine.RF_TWO_SETS, C.byref(s1), C.byref(empty), 64, p), (engine.RF_TWO_SETS, C.byref(s1), None, 64, p),
                 (engine.RF_ALL_PAIRS, C.byref(s1), C.byref(s2), 64, p), (engine.RF_ADJACENT, C.byref(s1), C.byref(s2), 64, p),
                 (engine.RF_ALL_PAIRS, C.byref(s1), None, 15, p), (engine.RF_ADJACENT, C.byref(s1), None, 2, p),
                 (engine.RF_TWO_SETS, C.byref(s1), C.byref(s2), 3, p), (7, C.byref(s1), None, 64, p)):
        assert L.mpf_rf_distances_set(eng.h, *args) == -2, args
        still_serves()
    assert L.mpf_rf_distances_set(eng.h, engine.RF_ALL_PAIRS, C.byref(s1), None, 16, p) == 0 and out[:16].tolist() == want.reshape(-1).tolist()
    nd, tot = C.c_int32(), C.c_int64()
    assert L.mpf_split_counts_set(eng.h, C.byref(empty), None, 0, None, None, C.byref(nd), C.byref(tot)) == -2
    with pytest.raises(ValueError):
        eng.split_support(rec)
    # the sizing protocol of the supports: a short cap writes the number alone
    f, nb, k = eng._lists(*good)
    m = C.c_int32()
    assert L.mpf_split_support_set(eng.h, C.byref(s1), None, k, f.ctypes.data, nb.ctypes.data, 3, None, None, None, C.byref(m), None) == 0
    assert m.value == n + k - 1
    del keep1, keep2


# ---------------------------------------------------------------- one size pin
def test_size_pin(tmp_path):
    """256 trees x 500 taxa, a quarter of them contracted, all pairs: 4 x 4 tiles, several words per row, deep stacks; against the
    host-only program's sum and a sample of entries from the witness"""
    src = os.path.join(ROOT, "mpboot_amd", "host", "split_lists_host_main.cpp")
    n, N = 500, 256
    rng = np.random.default_rng(11)
    backs = sw.related_trees(n, N, 77, 6)
    items = [lw.collapse(b, n, int(rng.integers(1, n - 2)), rng) if i % 4 == 1 else b for i, b in enumerate(backs)]
    items[5] = lw.star(n)
    eng = _eng(n)
    got, so = _rf(eng, items)
    assert (got == got.T).all() and (np.diag(got) == 0).all()
    pick = rng.integers(0, N, size=(40, 2)).tolist() + [[0, N - 1], [N - 1, N - 2]]
    need = sorted({i for p in pick for i in p})
    sets = dict(zip(need, lw.split_sets([so[i] for i in need], n)))
    for i, j in pick:
        assert got[i, j] == len(sets[i] ^ sets[j]), (i, j)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None
    exe = str(tmp_path / "split_lists_host")
    subprocess.check_call([cxx, "-std=c++17", "-O2", src, "-o", exe])
    r = subprocess.run([exe, "rf", lw.write_sets(str(tmp_path / "t.bin"), n, 0, items), "quiet"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(line.split() for line in r.stdout.splitlines())
    assert int(out["entries"]) == N * N and int(out["sum"]) == int(got.astype(np.int64).sum())
