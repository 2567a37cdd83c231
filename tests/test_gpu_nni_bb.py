"""The NNI hill climb under -bb (mpf_ufboot_optimize_nni, k_nni_eval_masks) against the witness in tests/nni_bb_witness.py:
IQTree::optimizeNNI with save_all_trees == 2, every evaluated NNI and every step's current tree through saveCurrentTree.
Everything is compared exactly: integers and the 64-bit state of the tie stream, no tolerance anywhere.  The inputs are those of
tests/nni_bb_cases.py, which tests/test_nni_bb_witness.py shows to exercise the update rule."""
import numpy as np
import pytest

from helpers import FIXTURES, load_fixture, same_topology
from nni_bb_cases import CASES, boot_samples, setup, start_tree
from nni_bb_witness import NniBbWitness, make
from oracle.search_slow import LONG_MAX

pytestmark = pytest.mark.gpu


def _engine(fx, keep_all=False, **kw):
    from mpboot_amd import engine
    return engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], keep_all=keep_all, **kw)


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


def _same_climb(e, w, got, want, n):
    assert got == want
    assert (e.get_tree() == np.array(w.back, dtype=np.int32)).all()
    assert [tuple(int(x) for x in m) for m in e.nni_moves()] == w.log
    _same_books(e, w, n)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tracked_climb_equals_the_witness(case):
    from mpboot_amd import engine
    fx, n, root, back, samples, w, cutoff = setup(case)
    e = _engine(fx, case.get("keep_all", False))
    e.seed_ties(engine.TIE_RANDOM, case["tie"])
    e.set_tree(back)
    e.ufboot_attach(samples)
    if w.mulhits:
        e.ufboot_set_mulhits(True)
    if w.cutoff_from_btrees:
        e.ufboot_set_cutoff_from_btrees(True)
    if cutoff:
        e.ufboot_set_cutoff(cutoff)
    r0, b0 = e.get_option("nni_rollbacks"), e.get_option("nni_booked")
    got = e.ufboot_optimize_nni(root, case["speednni"])
    want = w.optimize_nni(speednni=case["speednni"])
    _same_climb(e, w, got, want, n)
    assert e.get_option("nni_rollbacks") - r0 == w.rollbacks
    assert e.get_option("nni_booked") - b0 == len(w.calls) > 0
    assert w.ufb_draws > 0 or w.mulhits


def test_normal_ratchet_normal_then_spr_on_one_tracker():
    """three tracked NNI climbs on one tracker -- a short one, then one re-weighted as Alignment::createPerturbAlignment
    re-weights (booked under each tree's own length on the original alignment) under a cut-off set from the first climb's trees,
    then one back on the original weights -- and an SPR tracked climb behind them: the tracker's state survives every hand-over"""
    from mpboot_amd import engine
    fx = load_fixture("dna_clean")
    n = fx["codes_np"].shape[0]
    w0 = fx["weights_np"]
    samples = boot_samples(len(w0), 8, 21, fx["weights"])
    e = _engine(fx)
    w = make(fx, 31, samples)
    e.seed_ties(engine.TIE_RANDOM, 31)
    e.ufboot_attach(samples)
    starts = [start_tree(fx, ("random", s)) for s in (5, 6, 7)]
    # normal NNI climb, two steps: the samples hold trees of a climb under way
    e.set_tree(starts[0]); w.set_tree(starts[0])
    _same_climb(e, w, e.ufboot_optimize_nni(1, True, 2), w.optimize_nni(True, 2), n)
    n1 = len(w.treels_logl)
    # ratchet NNI climb under a cut-off: the best 3 % of what is booked so far
    cutoff = float(np.sort(np.array(w.treels_logl))[int(n1 * 0.97)])
    pert, _st = engine.iq_perturb_weights(w0, fx["informative"], 50, 1, 12345)
    assert (pert != w0).any() and not ((w0 > 0) & (pert <= 0)).any()
    e.ufboot_set_cutoff(cutoff); w.cutoff = cutoff
    e.set_weights(pert); w.set_weights(pert)
    assert w.ratchet
    e.set_tree(starts[1]); w.set_tree(starts[1])
    calls0 = len(w.calls)
    _same_climb(e, w, e.ufboot_optimize_nni(1, False), w.optimize_nni(False), n)
    # this climb's own candidates, under each one's own length on the original alignment: some pass the cut-off and are booked,
    # some fail, and some sample took one that passed
    mine = [(k, t) for k, _s, t in w.calls[calls0:] if k == "cand"]
    assert any(t is not None for _k, t in mine) and any(t is None for _k, t in mine)
    assert any(m and k == "cand" for m, (k, _s, _t) in zip(w.took[calls0:], w.calls[calls0:]))
    # back on the original weights, from the other root
    e.set_weights(w0); w.set_weights(w0)
    e.set_tree(starts[2]); w.set_tree(starts[2])
    w.root = n
    _same_climb(e, w, e.ufboot_optimize_nni(n, True), w.optimize_nni(True), n)
    # SPR behind
    assert e.optimize_spr(1, 3) == w.optimize(1, 3)
    _same_books(e, w, n)
    assert (e.get_tree() == np.array(w.back, dtype=np.int32)).all()


def test_nni_climb_behind_an_spr_climb():
    """the other direction of the hand-over: what an SPR tracked climb left in the tracker is what the NNI climb books into"""
    from mpboot_amd import engine
    fx = load_fixture("dna_ambig")
    n = fx["codes_np"].shape[0]
    samples = boot_samples(len(fx["weights"]), 8, 4, fx["weights"])
    e = _engine(fx)
    w = make(fx, 13, samples)
    e.seed_ties(engine.TIE_RANDOM, 13)
    e.ufboot_attach(samples)
    a, b = start_tree(fx, ("random", 8)), start_tree(fx, ("random", 9))
    e.set_tree(a); w.set_tree(a)
    assert e.optimize_spr(1, 2) == w.optimize(1, 2)
    _same_books(e, w, n)
    e.set_tree(b); w.set_tree(b)
    _same_climb(e, w, e.ufboot_optimize_nni(1, True), w.optimize_nni(True), n)
    assert len(w.calls) > 0


def test_no_hclimb1_bb_climbs_without_booking():
    from mpboot_amd import engine
    fx = load_fixture("dna_dups")
    n = fx["codes_np"].shape[0]
    w0 = fx["weights_np"]
    samples = boot_samples(len(w0), 8, 3, fx["weights"])
    e = _engine(fx)
    w = make(fx, 9, samples)
    e.seed_ties(engine.TIE_RANDOM, 9)
    e.ufboot_attach(samples)
    e.ufboot_set_ratchet_booking(False); w.ratchet_booking = False
    back = start_tree(fx, ("random", 1))
    e.set_tree(back); w.set_tree(back)
    _same_climb(e, w, e.ufboot_optimize_nni(1, True), w.optimize_nni(True), n)
    booked = len(w.treels_logl)
    assert booked > 0
    e.set_weights((w0 * 2).astype(np.int32)); w.set_weights(w0 * 2)
    e.set_tree(back); w.set_tree(back)
    _same_climb(e, w, e.ufboot_optimize_nni(1, True), w.optimize_nni(True), n)
    assert len(e.ufboot_tree_logl()) == booked


def test_1000_samples_on_the_synthetic_alignment():
    """200 x 10 000 DNA (the word-major copy, one word per lane), 1000 samples: two steps from a stepwise tree"""
    from mpboot_amd import engine, synth
    from oracle import pyoracle as po
    letters, _ = synth.synth_alignment(200, 10000, "DNA", 0.08, seed=4)
    codes = synth.letters_to_codes(letters, "DNA")
    o = po.Oracle(codes)
    o.stepwise(1)
    back = o.get_tree()
    P = codes.shape[1]
    samples = np.random.default_rng(7).multinomial(P, np.ones(P) / P, size=1000).astype(np.uint16)
    e = engine.FitchEngine(codes)
    w = NniBbWitness(codes, np.ones(P, dtype=np.int32), 0, o.informative().astype(bool), 5, samples)
    e.seed_ties(engine.TIE_RANDOM, 5)
    e.set_tree(back); w.set_tree(back)
    e.ufboot_attach(samples)
    got = e.ufboot_optimize_nni(1, True, 2)
    want = w.optimize_nni(True, 2)
    _same_climb(e, w, got, want, 200)
    assert w.ufb_draws > 0 and len(w.calls) >= 1 + 2 * 197


def _tile_cases():
    out = []
    for name in FIXTURES:
        tiles = (-1, 0, 1, 2, 4) if name.startswith("dna") else (-1,)      # (other alphabets run one word per lane whatever is asked)
        out += [(name, t) for t in tiles]
    return out


@pytest.mark.parametrize("name,tile", _tile_cases())
def test_mask_kernel_rows_give_every_swapped_trees_pattern_lengths(name, tile):
    """the kernel alone, in the shape the engine picks by default (nni_tile -1) and, on DNA, in every other shape it is compiled
    in (word-major copy, 1, 2 and 4 words per lane): pattern_pars(T) - h + c_k == compute_parsimony(swapped tree) per pattern,
    and the counts are those of the plain kernel"""
    from nni_witness import NniWitness
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    for keep_all in (False, True):
        e = _engine(fx, keep_all)
        e.set_option("nni_tile", tile)
        ref = _engine(fx, keep_all)
        for back in (start_tree(fx, ("random", 0)), start_tree(fx, ("stepwise", 1), keep_all)):
            for root in (1, n):
                e.set_tree(back)
                a, b, ln = e.nni_scores(root)
                a2, b2, ln2, terms = e.nni_pattern_terms(root)
                assert (a == a2).all() and (b == b2).all() and (ln == ln2).all()
                assert (e.get_tree() == back).all()
                _s, base = ref.compute_parsimony(back)
                w = NniWitness(back, n, None, root_taxon=root)
                for i in range(len(a)):
                    for k, mv in enumerate(w.branch_moves(int(a[i]), int(b[i]))):
                        w.swap(mv, log=False)
                        s, ptn = ref.compute_parsimony(w.back)
                        w.swap(mv, log=False)
                        got = base.astype(np.int64) - terms[i][0] + terms[i][1 + k]
                        assert (got == ptn).all(), (name, keep_all, root, i, k)
                        assert s == ln[i][k]


def test_refusals():
    from mpboot_amd import engine
    fx = load_fixture("dna_clean")
    P = len(fx["weights"])
    samples = boot_samples(P, 4, 5, fx["weights"])
    back = start_tree(fx, ("random", 0))

    def code(fn):
        with pytest.raises(engine.MpfError) as ei:
            fn()
        return ei.value.code

    e = _engine(fx)
    e.set_tree(back)
    assert code(lambda: e.ufboot_optimize_nni(1)) == -5                  # no tracker
    e2 = _engine(fx)
    e2.ufboot_attach(samples)
    assert code(lambda: e2.ufboot_optimize_nni(1)) == -5                 # no tree
    e.ufboot_attach(samples)
    assert code(lambda: e.optimize_nni(1)) == -6                         # the plain entry still refuses a tracker
    for root in (0, fx["codes_np"].shape[0] + 1):
        assert code(lambda: e.ufboot_optimize_nni(root)) == -2
    # the three optional rules: refused, not served wrongly
    for setter in (lambda x: x.ufboot_set_store_trees(True), lambda x: (x.ufboot_set_mulhits(True), x.ufboot_set_topboot(3)),
                   lambda x: x.ufboot_set_distinct_iter(2)):
        x = _engine(fx)
        x.set_tree(back)
        x.ufboot_attach(samples)
        setter(x)
        assert code(lambda: x.ufboot_optimize_nni(1)) == -6
        assert len(x.ufboot_tree_logl()) == 0 and (x.get_tree() == back).all()
    # a sample-sharded tracker
    import ctypes as C
    ex = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)(lambda *a: 1)
    sh = _engine(fx)
    sh.set_tree(back)
    sh.ufboot_attach(samples, shard=(0, 2), exchange=ex)
    assert code(lambda: sh.ufboot_optimize_nni(1)) == -6
    # the weighted engine
    cost = np.ones((4, 4), dtype=np.uint32) - np.eye(4, dtype=np.uint32)
    snk = _engine(fx, cost=cost)
    snk.set_tree(back)
    snk.ufboot_attach(samples)
    assert code(lambda: snk.ufboot_optimize_nni(1)) == -6
