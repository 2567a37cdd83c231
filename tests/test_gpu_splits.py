"""The summary of a -bb run on the engine (mpf_split_counts / mpf_split_support / mpf_consensus_tree / mpf_ufboot_summarize on
k_split_keys, k_split_insert, k_split_count, k_split_bits) against the witness of tests/splits_witness.py: collections.Counter over
trees.splits(back), weighted.  Exact integer equality everywhere; nothing is a tolerance."""
import numpy as np
import pytest

import splits_witness as sw
from helpers import load_fixture
from mpboot_amd import trees

pytestmark = pytest.mark.gpu

SIZES = (4, 5, 31, 32, 33, 64, 65, 97)      # the word boundaries of the sets: one split, first and last bit of a word


def _engine(n, P=64, seed=1):
    from mpboot_amd import engine
    rng = np.random.default_rng(seed)
    codes = (1 << rng.integers(0, 4, size=(n, P))).astype(np.uint8)
    return engine.FitchEngine(codes)


_ENGINES = {}


def _eng(n):
    if n not in _ENGINES:
        _ENGINES[n] = _engine(n)
    return _ENGINES[n]


def _as_pairs(bits, count):
    return [(sw.words_set(bits[i]), int(count[i])) for i in range(len(count))]


def _check_counts(eng, n, backs, weights=None):
    bits, count, total = eng.split_counts(backs, weights)
    c, t = sw.counts(backs, weights)
    assert total == t
    assert _as_pairs(bits, count) == sw.contract_order(c, n)
    assert eng.split_counts(backs, weights, counts_only=True) == (len(c), t)
    return c, t


@pytest.mark.parametrize("n", SIZES)
def test_word_boundary_sizes(n):
    rng = np.random.default_rng(40 + n)
    backs = [trees.random_topology(n, rng) for _ in range(10)] + [sw.caterpillar(n), sw.balanced(n)]
    eng = _eng(n)
    c, _ = _check_counts(eng, n, backs)
    assert eng.get_option("split_overflow") == 0
    assert len(c) >= n - 3


def test_weights():
    n = 33
    eng = _eng(n)
    rng = np.random.default_rng(7)
    backs = [trees.random_topology(n, rng) for _ in range(5)] + [sw.caterpillar(n)]
    backs.append(backs[1].copy())
    _check_counts(eng, n, backs, None)
    _check_counts(eng, n, backs, [1, 0, 3, 2, 0, 7, 4])
    _check_counts(eng, n, backs[:1], None)
    _check_counts(eng, n, backs[:1], [5])
    # a total above 2^31: the counts are 64-bit
    big = [2 ** 30, 2 ** 30, 2 ** 30, 2 ** 31 - 1, 1, 0, 2 ** 30]
    c, t = _check_counts(eng, n, backs, big)
    assert t > 2 ** 31 and max(c.values()) > 2 ** 31
    # every weight 0: nothing
    bits, count, total = eng.split_counts(backs[:2], [0, 0])
    assert len(count) == 0 and total == 0


def test_numbering_and_slot_order_do_not_matter():
    n = 40
    eng = _eng(n)
    names = ["t%d" % i for i in range(1, n + 1)]
    a = trees.random_topology(n, np.random.default_rng(12))
    # the same unrooted tree written from another tip: the taxa come in another order, so newick_to_back numbers the inner nodes
    # differently and the slots are rotated
    b = trees.newick_to_back(trees.back_to_newick(a, names, start_tip=17), names)
    assert (a != b).any() and trees.splits(a) == trees.splits(b)
    one = eng.split_counts([a])
    other = eng.split_counts([b])
    assert (one[0] == other[0]).all() and (one[1] == other[1]).all() and one[2] == other[2] == 1
    both = eng.split_counts([a, b])
    assert (both[0] == one[0]).all() and (both[1] == 2 * one[1]).all() and both[2] == 2
    assert len(one[1]) == n - 3


@pytest.fixture(scope="module")
def related():
    n = 40
    backs = sw.related_trees(n, 40, 21, 3)
    weights = [int(x) for x in np.random.default_rng(3).integers(0, 4, size=40)]
    return n, backs, weights, sw.counts(backs, weights)


def _check_support(eng, n, backs, weights, c, total, target):
    node1, node2, sup, t = eng.split_support(backs, target, weights)
    assert t == total
    eng.set_tree(target)
    a, b, _ = eng.branch_substitutions(1)
    assert (node1 == a).all() and (node2 == b).all()
    below = {}

    def tips(rec):
        v = rec // 3
        if v <= n:
            return frozenset([v])
        below[v] = tips(int(target[trees.nxt(rec)])) | tips(int(target[trees.nxt(trees.nxt(rec))]))
        return below[v]

    tips(int(target[3]))
    want = []
    for u, v in zip(node1, node2):
        inner = u > n and v > n
        want.append(c.get(below[int(v)], 0) if inner else -1)
    assert sup.tolist() == want
    assert sum(1 for x in want if x >= 0) == n - 3
    return want


def _related_checks(eng, related):
    n, backs, weights, (c, total) = related
    out = [eng.split_counts(backs, weights)]
    assert _as_pairs(out[0][0], out[0][1]) == sw.contract_order(c, n) and out[0][2] == total
    inside = _check_support(eng, n, backs, weights, c, total, backs[4])
    assert max(inside) > 0
    stranger = trees.random_topology(n, np.random.default_rng(77))
    outside = _check_support(eng, n, backs, weights, c, total, stranger)
    assert 0 in outside                       # a branch it shares with nobody
    return out[0], inside, outside


def test_related_trees(related):
    n = related[0]
    eng = _eng(n)
    _related_checks(eng, related)
    assert eng.get_option("split_overflow") == 0


def test_overflow_path(related):
    """4-bit keys: nearly every cluster collides with its slot's representative and the overflow list carries the result"""
    n = related[0]
    eng = _eng(n)
    full = _related_checks(eng, related)
    eng.set_option("split_key_bits", 4)
    try:
        assert eng.get_option("split_key_bits") == 4
        masked = _related_checks(eng, related)
        assert eng.get_option("split_overflow") > 0
        n_, backs, weights, _ = related
        cons = eng.consensus_tree(backs, weights, 0.5)
        assert eng.get_option("split_overflow") > 0
    finally:
        eng.set_option("split_key_bits", 64)
    assert (masked[0][0] == full[0][0]).all() and (masked[0][1] == full[0][1]).all() and masked[1:] == full[1:]
    again = eng.consensus_tree(backs, weights, 0.5)
    assert all((x == y).all() for x, y in zip(cons[:3], again[:3])) and cons[3] == again[3]
    assert eng.get_option("split_overflow") == 0


def _check_consensus(eng, n, backs, weights, threshold):
    first, nbr, sup, total = eng.consensus_tree(backs, weights, threshold)
    c, t = sw.counts(backs, weights)
    assert total == t
    below = sw.list_splits(first, nbr, n)
    got = {v: s for v, s in below.items() if len(s) < n - 1}
    kept = sw.greedy(sw.contract_order(c, n), t, threshold, n)      # the greedy pass over the witness in the contract order
    assert set(got.values()) == {s for s, _ in kept}
    if threshold >= 0.5:
        assert set(got.values()) == {s for s, k in c.items() if k > threshold * t and 2 * k > t}
    assert len(sup) == len(first) - 1 and sup[0] == -1
    for v, s in got.items():
        assert sup[v - n - 1] == c[s]
    assert (first.tolist(), nbr.tolist(), sup.tolist()) == sw.build_lists(kept, n)
    length = eng.polytomy_parsimony(first, nbr)                     # the lists are what mpf_polytomy_parsimony takes
    assert length > 0
    return kept, length


def test_consensus(related):
    n, backs, weights, (c, total) = related
    eng = _eng(n)
    majority, _ = _check_consensus(eng, n, backs, weights, 0.5)
    greedy, _ = _check_consensus(eng, n, backs, weights, 0.0)
    assert 0 < len(majority) < n - 3          # a majority split, and a true polytomy
    assert len(greedy) >= len(majority)
    # farther apart: the majority rule leaves less
    far = sw.related_trees(n, 40, 22, 12)
    kept_far, _ = _check_consensus(eng, n, far, None, 0.5)
    assert len(kept_far) < n - 3
    _check_consensus(eng, n, far, None, 0.0)
    _check_consensus(eng, n, far, None, 0.75)


def test_consensus_of_one_tree_is_that_tree():
    n = 40
    eng = _eng(n)
    t = trees.random_topology(n, np.random.default_rng(5))
    for threshold in (0.0, 0.5):
        kept, length = _check_consensus(eng, n, [t] * 40, None, threshold)
        assert len(kept) == n - 3
        assert length == eng.score_tree(t)
        first, nbr, sup, total = eng.consensus_tree([t] * 40, None, threshold)
        assert trees.splits(trees.lists_to_back(first, nbr, n)) == trees.splits(t)
        assert sup[1:].tolist() == [40] * (n - 3) and total == 40


@pytest.mark.parametrize("rule", ("default", "mulhits"))
def test_tracker(rule):
    from mpboot_amd import engine
    fx = load_fixture("dna_48")
    n, B = fx["n"], 64
    w0 = fx["weights_np"]
    rng = np.random.default_rng(29)
    samples = rng.multinomial(int(w0.sum()), w0 / w0.sum(), size=B).astype(np.uint16)
    e = engine.FitchEngine(fx["codes_np"], w0, datatype=fx["datatype"])
    with pytest.raises(engine.MpfError) as err:
        e.ufboot_summarize()
    assert err.value.code == -5                # MPF_E_STATE without a tracker
    start = np.array(fx["trees"][2]["back"], dtype=np.int32)
    e.seed_ties(engine.TIE_RANDOM, 31)
    e.ufboot_attach(samples)
    if rule == "mulhits":
        e.ufboot_set_mulhits(True)
    e.set_tree(start)
    e.optimize_spr(1, 6)
    best = e.get_tree()
    tally = {}
    if rule == "default":
        for t in e.ufboot_state()[2]:
            tally[int(t)] = tally.get(int(t), 0) + 1
    else:
        for b in range(B):
            hits = e.ufboot_sample_trees(b)
            for t in hits:
                tally[int(t)] = tally.get(int(t), 0) + B // len(hits)
    idx = sorted(tally)
    backs = [e.ufboot_tree(t) for t in idx]
    weights = [tally[t] for t in idx]
    ti, tw, tb = e.ufboot_summary_trees()
    assert ti.tolist() == idx and tw.tolist() == weights and (tb == np.asarray(backs)).all()
    s = e.ufboot_summarize(target=best, threshold=0.5)
    bits, count, total = e.split_counts(backs, weights)
    assert (s["bits"] == bits).all() and (s["count"] == count).all() and s["total_weight"] == total == sum(weights)
    assert s["n_trees"] == len(idx)
    a, b, sup, _ = e.split_support(backs, best, weights)
    assert (s["node1"] == a).all() and (s["node2"] == b).all() and (s["support"] == sup).all()
    first, nbr, isup, _ = e.consensus_tree(backs, weights, 0.5)
    assert (s["first"] == first).all() and (s["nbr"] == nbr).all() and (s["support_of_inner"] == isup).all()
    c, t = sw.counts(backs, weights)
    assert _as_pairs(bits, count) == sw.contract_order(c, n)
    from mpboot_amd import bootstrap
    r = bootstrap.bb_summary(e, best, 0.5)
    assert (r["support"] == sup).all() and r["consensus_length"] == e.polytomy_parsimony(first, nbr) and r["total_weight"] == total
    names = ["t%d" % i for i in range(1, n + 1)]
    assert trees.lists_to_newick(first, nbr, names, isup).count("(") == len(first) - 1
    if rule == "default":
        with pytest.raises(engine.MpfError) as err:
            e.ufboot_summarize(rule=engine.SUMMARY_MULHITS)
        assert err.value.code == -5


def test_refusals():
    from mpboot_amd import engine
    n = 12
    eng = _eng(n)
    rng = np.random.default_rng(2)
    good = [trees.random_topology(n, rng) for _ in range(3)]

    def refused(backs, weights=None, target=None):
        with pytest.raises(engine.MpfError) as err:
            if target is None:
                eng.split_counts(backs, weights)
            else:
                eng.split_support(backs, target, weights)
        assert err.value.code == -2            # MPF_E_INVALID
        if target is None:
            with pytest.raises(engine.MpfError):
                eng.consensus_tree(backs, weights, 0.5)

    # an incomplete tree: a tip that hangs on nothing
    partial = good[0].copy()
    r = int(partial[3 * n])
    partial[3 * n] = partial[r] = -1
    refused([good[0], partial])
    refused(good[:1], target=partial)
    # wrong n: a tree on another number of taxa
    other = trees.random_topology(n + 1, rng)
    refused([good[0], other[:len(good[0])]])
    refused(good[:1], target=other[:len(good[0])])
    # records that link both ways everywhere but close a cycle: not ONE tree (the walk of k_split_keys is bounded by a tree's
    # node counts and reports it)
    for t in good:
        refused([good[0], sw.cyclic_records(t, n)])
    refused(good[:1], target=sw.cyclic_records(good[1], n))
    # a negative weight
    refused(good, [1, -1, 1])
    with pytest.raises(engine.MpfError):
        eng.consensus_tree(good, None, 1.5)
    # cap = 0: counts only
    c, t = sw.counts(good)
    assert eng.split_counts(good, counts_only=True) == (len(c), t)
    _check_counts(eng, n, good)                # and the engine still serves
