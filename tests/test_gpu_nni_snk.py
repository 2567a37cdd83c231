"""The NNI hill climb on the weighted engine (option "nni_weighted": mpf_optimize_nni / mpf_nni_scores / mpf_get_nni_moves on
k_snk_nni_eval) against the witness of IQTree::optimizeNNI on a ParsTree in tests/nni_snk_witness.py.  Everything is exact equality.

Size pin: the full climb against the witness at 120 x 3000 protein and 200 x 10 000 DNA (test_climb_at_size), capped at two steps
from a random tree -- the witness takes 2-4 s there, a climb to its end from such a tree half a minute."""
import ctypes as C

import numpy as np
import pytest

import nni_snk_cases as cases
from nni_snk_witness import SnkNniWitness, SnkScorer

pytestmark = pytest.mark.gpu

TAXA = (4, 5, 6, 16, 40)                                  # 4: one inner branch
COUNTS = (1, 63, 64, 65, 127, 128, 129, 257)              # kept patterns: the tile edges of 32-bit (64 per wave) and 16-bit costs (128)


def _alignment(n, P, protein, seed):
    """random tip codes with ambiguity and unknowns, weights 1 .. 5; keep_all engines keep every pattern"""
    rng = np.random.default_rng(seed)
    if protein:
        codes = rng.integers(0, 20, size=(n, P))
        odd = rng.integers(20, 23, size=(n, P))
    else:
        codes = 1 << rng.integers(0, 4, size=(n, P))
        odd = rng.integers(1, 16, size=(n, P))
    codes = np.where(rng.random((n, P)) < 0.1, odd, codes).astype(np.uint8)
    return codes, rng.integers(1, 6, size=P).astype(np.int32)


def _engine(codes, weights, protein, cost, keep_all=True):
    from mpboot_amd import engine
    e = engine.FitchEngine(codes, weights, datatype=engine.AA if protein else engine.DNA, keep_all=keep_all, cost=cost)
    e.set_option("nni_weighted", 1)
    return e


def _scores(eng, root):
    a, b, ln = eng.nni_scores(root)
    return [(int(x), int(y), int(l[0]), int(l[1])) for x, y, l in zip(a, b, ln)]


def _length_at(eng, root):
    """mpf_compute_parsimony_at: every vector made again, the tree evaluated at the root leaf's edge"""
    from mpboot_amd import engine
    s = C.c_uint32()
    rc = engine.load_library().mpf_compute_parsimony_at(eng.h, None, root, C.byref(s), None)
    assert rc == 0
    return s.value


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_nni_scores_equal_the_witness(protein, P):
    """the kernel alone: both moves of every inner branch, 16-bit and 32-bit costs, symmetric and non-symmetric matrices"""
    from mpboot_amd import trees
    S = 20 if protein else 4
    for i, n in enumerate(TAXA):
        kind = ("metric", "asym")[(i + COUNTS.index(P)) % 2]
        cost = cases.cost_of(kind, S, seed=7 + i)
        codes, weights = _alignment(n, P, protein, 100 * P + n)
        back = trees.random_topology(n, np.random.default_rng(n + P))
        sc = SnkScorer(codes, weights, cost, protein=protein)
        eng = _engine(codes, weights, protein, cost)
        assert eng.num_informative == P
        for short in (1, 0):
            eng.set_option("sankoff_short", short)
            eng.set_tree(back)
            for root in (1, n):
                want = SnkNniWitness(back, n, sc, root_taxon=root).scores()
                assert len(want) == n - 3
                assert _scores(eng, root) == want, (n, kind, short, root)
            assert (eng.get_tree() == back).all()


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "aa"])
def test_wide_addressing(protein):
    """option force_big: 64-bit pointers per row, what a store of 4 GiB and more takes"""
    from mpboot_amd import trees
    n, P = 16, 129
    cost = cases.cost_of("asym", 20 if protein else 4)
    codes, weights = _alignment(n, P, protein, 5)
    back = trees.random_topology(n, np.random.default_rng(2))
    want = SnkNniWitness(back, n, SnkScorer(codes, weights, cost, protein=protein)).scores()
    eng = _engine(codes, weights, protein, cost)
    eng.set_option("force_big", 1)
    for short in (1, 0):
        eng.set_option("sankoff_short", short)
        eng.set_tree(back)
        assert _scores(eng, 1) == want


@pytest.mark.parametrize("name", ["morph32", "morph32_40"])
def test_32_state_kernels_equal_the_oracle(name):
    """multistate data under a matrix runs the 32-row kernels; with a symmetric matrix the length does not depend on the root edge,
    so NniWitness over the pinned oracle's weighted score_tree (every swap done, the whole tree scored) is the reference"""
    from helpers import load_fixture
    from mpboot_amd import engine, trees
    from nni_witness import NniWitness
    from oracle import pyoracle as po
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    cost = cases.metric(32, 4)
    o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
    eng = engine.FitchEngine(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"], cost=cost)
    assert eng.get_option("kernel_states") == 32
    eng.set_option("nni_weighted", 1)
    back = trees.random_topology(n, np.random.default_rng(1))
    want = NniWitness(back, n, lambda b: o.score_tree(b)).scores()
    for short in (1, 0):
        eng.set_option("sankoff_short", short)
        eng.set_tree(back)
        assert _scores(eng, 1) == want


def _compare_climb(eng, case, speednni, max_steps=None):
    w = cases.witness(case, speednni, max_steps=max_steps)
    _fx, _cost, n, root, back, _sc = cases.setup(case)
    steps = case["steps"] if max_steps is None else max_steps
    eng.set_tree(back)
    k0, r0 = eng.get_option("nni_kept_worse"), eng.get_option("nni_rollbacks")
    got = eng.optimize_nni(root, speednni, steps)
    assert got == w.result
    assert (eng.get_tree() == w.back).all()
    assert [tuple(int(x) for x in m) for m in eng.nni_moves()] == w.log
    assert eng.get_option("nni_kept_worse") - k0 == w.kept_worse
    assert eng.get_option("nni_rollbacks") == r0
    # the views the climb refreshed after its swaps against every vector made again
    assert _length_at(eng, root) == got[0]
    assert (eng.get_tree() == w.back).all()
    return w


@pytest.mark.parametrize("speednni", [True, False])
@pytest.mark.parametrize("case", cases.CASES, ids=[c["id"] for c in cases.CASES])
def test_optimize_nni_equals_the_witness(case, speednni):
    fx, cost, _n, _root, _back, _sc = cases.setup(case)
    eng = _engine(fx["codes_np"], fx["weights_np"], fx["S"] == 20, cost, keep_all=False)
    w = _compare_climb(eng, case, speednni)
    if case["cost"] != "asym":
        assert eng.score_tree() == w.result[0]            # a symmetric matrix: the same length at taxon 1's edge
    # 32-bit costs, and a cap below the natural end
    eng.set_option("sankoff_short", 0)
    _compare_climb(eng, case, speednni, max_steps=2)


@pytest.mark.parametrize("nt,L,alpha,kind", [(120, 3000, "AA", "metric"), (200, 10000, "DNA", "asym")])
def test_climb_at_size(nt, L, alpha, kind):
    from mpboot_amd import synth, trees
    letters, _ = synth.synth_alignment(nt, L, alpha, 0.08, seed=4)
    codes = synth.letters_to_codes(letters, alpha)
    protein = alpha == "AA"
    cost = cases.cost_of(kind, 20 if protein else 4)
    weights = np.ones(codes.shape[1], dtype=np.int32)
    back = trees.random_topology(nt, np.random.default_rng(5))
    w = SnkNniWitness(back, nt, SnkScorer(codes, weights, cost, protein=protein))
    want = w.optimize(True, max_steps=2)
    eng = _engine(codes, weights, protein, cost, keep_all=False)
    eng.set_tree(back)
    assert eng.optimize_nni(1, True, 2) == want
    assert (eng.get_tree() == w.back).all()
    assert [tuple(int(x) for x in m) for m in eng.nni_moves()] == w.log
    assert _length_at(eng, 1) == want[0]


def test_what_stays_refused():
    from mpboot_amd import engine, trees
    fx, cost, n, _root, back, _sc = cases.setup(cases.CASES[0])
    snk = engine.FitchEngine(fx["codes_np"], fx["weights_np"], cost=cost)
    snk.set_tree(back)
    assert snk.get_option("nni_weighted") == 0
    for call in (lambda: snk.optimize_nni(1), lambda: snk.nni_scores(1)):          # option off: as before
        with pytest.raises(engine.MpfError) as ei:
            call()
        assert ei.value.code == -6
    snk.set_option("nni_weighted", 1)
    assert snk.get_option("nni_weighted") == 1
    with pytest.raises(engine.MpfError) as ei:                                     # the mask rows are Fitch joins
        snk.nni_pattern_terms(1)
    assert ei.value.code == -6
    P = fx["codes_np"].shape[1]
    samples = np.random.default_rng(5).multinomial(P, np.ones(P) / P, size=4).astype(np.uint16)
    snk.ufboot_attach(samples)
    for call in (lambda: snk.optimize_nni(1), lambda: snk.ufboot_optimize_nni(1)):  # a tracker attached; the tracked weighted climb
        with pytest.raises(engine.MpfError) as ei:
            call()
        assert ei.value.code == -6
    snk.ufboot_detach()
    assert (snk.get_tree() == back).all()
    snk.optimize_nni(1)                                                            # ... and served again without it
    # a Fitch engine takes the option and is not changed by it
    f0 = engine.FitchEngine(fx["codes_np"], fx["weights_np"])
    f1 = engine.FitchEngine(fx["codes_np"], fx["weights_np"])
    f1.set_option("nni_weighted", 1)
    res = []
    for f in (f0, f1):
        f.set_tree(back)
        res.append((f.optimize_nni(1), f.get_tree().tolist(), f.nni_moves().tolist(), f.get_option("nni_kept_worse")))
    assert res[0] == res[1] and res[0][3] == 0
