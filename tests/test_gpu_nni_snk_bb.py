"""The NNI hill climb on the weighted engine under -bb (options "nni_weighted" + "nni_weighted_tracked": mpf_ufboot_optimize_nni on
k_snk_nni_eval_vals, mpf_nni_pattern_lengths) against the witness in tests/nni_snk_bb_witness.py: IQTree::optimizeNNI on a ParsTree
with save_all_trees == 2.  Everything is compared exactly: integers and the 64-bit state of the tie stream, no tolerance anywhere.
The inputs are those of tests/nni_snk_bb_cases.py, which tests/test_nni_snk_bb_witness.py shows to exercise the update rule.

Size pin: 120 x 3000 protein with 16 samples from a random tree, capped at one step (one full evaluation of 117 branches)."""
import ctypes as C

import numpy as np
import pytest

import nni_snk_cases as snk_cases
from helpers import load_fixture
from nni_bb_cases import boot_samples
from nni_snk_bb_cases import CASES, climbed, start_tree
from nni_snk_bb_witness import RowScorer, SnkNniBbWitness, make
from nni_snk_witness import SnkNniWitness
from nni_witness import NniWitness
from test_gpu_nni_bb import _same_books, _same_climb

pytestmark = pytest.mark.gpu

TAXA = (4, 5, 6, 16)                                      # 4: one inner branch
COUNTS = (1, 63, 64, 65, 127, 128, 129, 257)              # kept patterns: the tile edges of 32-bit (64 per wave) and 16-bit costs (128)


def _alignment(n, P, protein, seed):
    """P patterns the engine keeps (two definite states at least; ambiguity and unknowns among the rest) with three it drops (one
    state throughout) in front, in the middle and behind; weights 1 .. 5"""
    rng = np.random.default_rng(seed)
    if protein:
        codes = rng.integers(0, 20, size=(n, P))
        odd = rng.integers(20, 23, size=(n, P))
        codes[0], codes[1] = 3, 7
        flat = np.full((n, 1), 5)
    else:
        codes = 1 << rng.integers(0, 4, size=(n, P))
        odd = rng.integers(1, 16, size=(n, P))
        codes[0], codes[1] = 1, 4
        flat = np.full((n, 1), 2)
    mixed = np.where(rng.random((n, P)) < 0.1, odd, codes)
    mixed[:2] = codes[:2]
    h = P // 2
    codes = np.concatenate([flat, mixed[:, :h], flat, mixed[:, h:], flat], axis=1).astype(np.uint8)
    return codes, rng.integers(1, 6, size=P + 3).astype(np.int32)


def _engine(codes, weights, datatype, cost):
    from mpboot_amd import engine
    e = engine.FitchEngine(codes, weights, datatype=datatype, cost=cost)
    e.set_option("nni_weighted", 1)
    e.set_option("nni_weighted_tracked", 1)
    return e


def _fx_engine(fx, cost, weights=None):
    return _engine(fx["codes_np"], fx["weights_np"] if weights is None else weights, fx["datatype"], cost)


def _witness_rows(sc, back, n, root):
    """row 0 the current tree at the root leaf, row 1 + 2 i + k move k of branch i at its branch; and the lengths"""
    w = NniWitness(back, n, None, root_taxon=root)
    rows, lens = [sc.root_row(back, root)], []
    for v1, v2 in w.full_order():
        for mv in w.branch_moves(v1, v2):
            w.swap(mv, log=False)
            rows.append(sc.edge_row(w.back, v1, v2))
            lens.append(sc.edge_length(w.back, v1, v2))
            w.swap(mv, log=False)
    return np.array(rows), lens


def _check_rows(eng, sc, back, n, root, tag):
    want, lens = _witness_rows(sc, back, n, root)
    a, b, ln, rows = eng.nni_pattern_lengths(root)
    a2, b2, ln2 = eng.nni_scores(root)
    assert (a == a2).all() and (b == b2).all() and (ln == ln2).all(), tag
    assert ln.reshape(-1).tolist() == lens, tag
    assert rows.dtype == np.uint16 and rows.shape == want.shape, tag
    assert (rows == want).all(), tag


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_pattern_lengths_equal_the_witness_rows(protein, P):
    """the kernel alone: both rows of every inner branch and the current tree's, 16-bit and 32-bit costs, symmetric and
    non-symmetric matrices, both roots, weights that are not 1, patterns the engine drops"""
    from mpboot_amd import trees
    S = 20 if protein else 4
    for i, n in enumerate(TAXA):
        kind = ("metric", "asym")[(i + COUNTS.index(P)) % 2]
        cost = snk_cases.cost_of(kind, S, seed=7 + i)
        codes, weights = _alignment(n, P, protein, 100 * P + n)
        back = trees.random_topology(n, np.random.default_rng(n + P))
        sc = RowScorer(codes, weights, cost, int(protein))
        eng = _engine(codes, weights, int(protein), cost)
        assert eng.num_informative == P
        for short in (1, 0):
            eng.set_option("sankoff_short", short)
            eng.set_tree(back)
            for root in (1, n):
                _check_rows(eng, sc, back, n, root, (n, kind, short, root))
            assert (eng.get_tree() == back).all()


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_pattern_lengths_with_wide_addressing(protein):
    """option force_big: 64-bit pointers per row, what a store of 4 GiB and more takes"""
    from mpboot_amd import trees
    n, P = 16, 129
    cost = snk_cases.cost_of("asym", 20 if protein else 4)
    codes, weights = _alignment(n, P, protein, 5)
    back = trees.random_topology(n, np.random.default_rng(2))
    sc = RowScorer(codes, weights, cost, int(protein))
    eng = _engine(codes, weights, int(protein), cost)
    eng.set_option("force_big", 1)
    for short in (1, 0):
        eng.set_option("sankoff_short", short)
        eng.set_tree(back)
        _check_rows(eng, sc, back, n, n, short)


@pytest.mark.parametrize("kind", ["metric", "asym"])
def test_pattern_lengths_on_the_32_row_kernels(kind):
    from mpboot_amd import trees
    fx = load_fixture("morph32")
    n = fx["codes_np"].shape[0]
    cost = snk_cases.cost_of(kind, 32)
    eng = _fx_engine(fx, cost)
    assert eng.get_option("kernel_states") == 32
    sc = RowScorer(fx["codes_np"], fx["weights_np"], cost, fx["datatype"])
    back = trees.random_topology(n, np.random.default_rng(1))
    for short in (1, 0):
        eng.set_option("sankoff_short", short)
        eng.set_tree(back)
        for root in (1, n):
            _check_rows(eng, sc, back, n, root, (short, root))


def _attach(e, w, samples, tie, cutoff=0.0):
    from mpboot_amd import engine
    e.seed_ties(engine.TIE_RANDOM, tie)
    e.ufboot_attach(samples)
    if w.mulhits:
        e.ufboot_set_mulhits(True)
    if w.cutoff_from_btrees:
        e.ufboot_set_cutoff_from_btrees(True)
    if cutoff:
        e.ufboot_set_cutoff(cutoff)


@pytest.mark.parametrize("cap", [None, 3], ids=["to-the-end", "cap-3"])
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tracked_climb_equals_the_witness(case, cap):
    (fx, cost, n, root, back, samples, w, cutoff), want = climbed(case["id"], cap)
    e = _fx_engine(fx, cost)
    e.set_tree(back)
    _attach(e, w, samples, case["tie"], cutoff)
    k0, r0, b0 = e.get_option("nni_kept_worse"), e.get_option("nni_rollbacks"), e.get_option("nni_booked")
    got = e.ufboot_optimize_nni(root, case["speednni"], case.get("steps", 50) if cap is None else cap)
    _same_climb(e, w, got, want, n)
    assert e.get_option("nni_kept_worse") - k0 == w.kept_worse
    assert e.get_option("nni_rollbacks") == r0
    assert e.get_option("nni_booked") - b0 == len(w.calls) > 0


def test_normal_ratchet_normal_then_spr_on_one_tracker():
    """three tracked NNI climbs on one tracker -- a short one, then one re-weighted as Alignment::createPerturbAlignment re-weights
    (booked under each tree's own row times the original frequencies) under a cut-off set from the first climb's trees, then one
    back on the original weights from the other root -- and a weighted tracked SPR climb behind them.  A symmetric matrix: the SPR
    climb's rows do not depend on the edge they are taken at, so SlowSearch.optimize on the witness's scorer is its reference"""
    from mpboot_amd import engine
    fx = load_fixture("dna_clean")
    n = fx["codes_np"].shape[0]
    w0 = fx["weights_np"]
    cost = snk_cases.cost_of("metric", 4)
    samples = boot_samples(len(w0), 8, 21, fx["weights"])
    e = _fx_engine(fx, cost)
    w = make(fx, cost, 31, samples)
    _attach(e, w, samples, 31)
    starts = [start_tree(fx, s) for s in (5, 6, 7)]
    e.set_tree(starts[0]); w.set_tree(starts[0])
    _same_climb(e, w, e.ufboot_optimize_nni(1, True, 2), w.optimize_nni(True, 2), n)
    n1 = len(w.treels_logl)
    cutoff = float(np.sort(np.array(w.treels_logl))[int(n1 * 0.97)])
    pert, _st = engine.iq_perturb_weights(w0, fx["informative"], 50, 1, 12345)
    assert (pert != w0).any() and not ((w0 > 0) & (pert <= 0)).any()
    e.ufboot_set_cutoff(cutoff); w.cutoff = cutoff
    e.set_weights(pert); w.set_weights(pert)
    assert w.ratchet
    e.set_tree(starts[1]); w.set_tree(starts[1])
    calls0 = len(w.calls)
    _same_climb(e, w, e.ufboot_optimize_nni(1, False), w.optimize_nni(False), n)
    mine = [(k, t) for k, _s, t in w.calls[calls0:] if k == "cand"]
    assert any(t is not None for _k, t in mine) and any(t is None for _k, t in mine)
    # ... each booked under its own row times the original frequencies, not under the length the climb saw
    booked = [(r, c) for r, c in zip(w.rows[calls0:], w.calls[calls0:]) if c[2] is not None]
    assert all(w.treels_logl[c[2]] == -float((r[3] * w0).sum()) for r, c in booked)
    assert any(int((r[3] * w0).sum()) != r[2] for r, _c in booked)
    e.set_weights(w0); w.set_weights(w0)
    e.set_tree(starts[2]); w.set_tree(starts[2])
    w.root = n
    _same_climb(e, w, e.ufboot_optimize_nni(n, True), w.optimize_nni(True), n)
    # SPR behind
    w.edge = None
    assert e.optimize_spr(1, 3) == w.optimize(1, 3)
    _same_books(e, w, n)
    assert (e.get_tree() == np.array(w.back, dtype=np.int32)).all()


def test_no_hclimb1_bb_climbs_without_booking():
    fx = load_fixture("dna_dups")
    n = fx["codes_np"].shape[0]
    w0 = fx["weights_np"]
    cost = snk_cases.cost_of("asym", 4)
    samples = boot_samples(len(w0), 8, 3, fx["weights"])
    e = _fx_engine(fx, cost)
    w = make(fx, cost, 9, samples)
    _attach(e, w, samples, 9)
    e.ufboot_set_ratchet_booking(False); w.ratchet_booking = False
    back = start_tree(fx, 1)
    e.set_tree(back); w.set_tree(back)
    _same_climb(e, w, e.ufboot_optimize_nni(1, True, 4), w.optimize_nni(True, 4), n)
    booked = len(w.treels_logl)
    assert booked > 0
    e.set_weights((w0 * 2).astype(np.int32)); w.set_weights(w0 * 2)
    e.set_tree(back); w.set_tree(back)
    b0 = len(w.calls)
    got = e.ufboot_optimize_nni(1, True, 4)
    _same_climb(e, w, got, w.optimize_nni(True, 4), n)
    assert len(e.ufboot_tree_logl()) == booked and all(t is None for _k, _s, t in w.calls[b0:])
    # ... and it is the plain weighted climb
    p = SnkNniWitness(back, n, w.scorer)
    assert p.optimize(True, 4) == got and p.log == w.log


def test_refusals():
    from mpboot_amd import engine
    fx = load_fixture("dna_clean")
    n = fx["codes_np"].shape[0]
    cost = snk_cases.cost_of("tstv", 4)
    samples = boot_samples(len(fx["weights"]), 4, 5, fx["weights"])
    back = start_tree(fx, 0)

    def code(fn):
        with pytest.raises(engine.MpfError) as ei:
            fn()
        return ei.value.code

    # the new option off: every refusal as before
    snk = engine.FitchEngine(fx["codes_np"], fx["weights_np"], cost=cost)
    snk.set_tree(back)
    assert snk.get_option("nni_weighted_tracked") == 0
    snk.set_option("nni_weighted", 1)
    assert code(lambda: snk.nni_pattern_lengths(1)) == -6
    snk.ufboot_attach(samples)
    assert code(lambda: snk.ufboot_optimize_nni(1)) == -6
    assert code(lambda: snk.optimize_nni(1)) == -6
    # ... on: the tracker forms the Fitch tracked climb refuses, the plain entry with a tracker, the Fitch rows
    for setter in (lambda x: x.ufboot_set_store_trees(True), lambda x: (x.ufboot_set_mulhits(True), x.ufboot_set_topboot(3)),
                   lambda x: x.ufboot_set_distinct_iter(2)):
        x = _fx_engine(fx, cost)
        x.set_tree(back)
        x.ufboot_attach(samples)
        setter(x)
        assert code(lambda: x.ufboot_optimize_nni(1)) == -6
        assert len(x.ufboot_tree_logl()) == 0 and (x.get_tree() == back).all()
    ex = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)(lambda *a: 1)
    sh = _fx_engine(fx, cost)
    sh.set_tree(back)
    sh.ufboot_attach(samples, shard=(0, 2), exchange=ex)
    assert code(lambda: sh.ufboot_optimize_nni(1)) == -6
    e = _fx_engine(fx, cost)
    assert e.get_option("nni_weighted_tracked") == 1
    assert code(lambda: e.ufboot_optimize_nni(1)) == -5                  # no tracker
    e.ufboot_attach(samples)
    assert code(lambda: e.ufboot_optimize_nni(1)) == -5                  # no tree
    e.set_tree(back)
    assert code(lambda: e.optimize_nni(1)) == -6
    assert code(lambda: e.nni_pattern_terms(1)) == -6
    for root in (0, n + 1):
        assert code(lambda: e.ufboot_optimize_nni(root)) == -2
    e.ufboot_detach()
    p = SnkNniWitness(back, n, RowScorer(fx["codes_np"], fx["weights_np"], cost))
    assert e.optimize_nni(1) == p.optimize() and (e.get_tree() == p.back).all()   # served again without it
    # a Fitch engine takes the option, is not changed by it, and has no such rows
    f = engine.FitchEngine(fx["codes_np"], fx["weights_np"])
    f.set_option("nni_weighted", 1)
    f.set_option("nni_weighted_tracked", 1)
    f.set_tree(back)
    assert code(lambda: f.nni_pattern_lengths(1)) == -6
    f0 = engine.FitchEngine(fx["codes_np"], fx["weights_np"])
    f0.set_tree(back)
    assert f.optimize_nni(1) == f0.optimize_nni(1) and (f.get_tree() == f0.get_tree()).all()


def test_one_step_at_size():
    from mpboot_amd import synth, trees
    nt, L = 120, 3000
    letters, _ = synth.synth_alignment(nt, L, "AA", 0.08, seed=4)
    codes = synth.letters_to_codes(letters, "AA")
    cost = snk_cases.cost_of("metric", 20)
    P = codes.shape[1]
    weights = np.ones(P, dtype=np.int32)
    samples = np.random.default_rng(7).multinomial(P, np.ones(P) / P, size=16).astype(np.uint16)
    back = trees.random_topology(nt, np.random.default_rng(5))
    w = SnkNniBbWitness(codes, weights, 1, cost, 5, samples)
    w.set_tree(back)
    want = w.optimize_nni(True, 1)
    e = _engine(codes, weights, 1, cost)
    e.set_tree(back)
    _attach(e, w, samples, 5)
    _same_climb(e, w, e.ufboot_optimize_nni(1, True, 1), want, nt)
    assert len(w.calls) == 1 + 2 * (nt - 3)
