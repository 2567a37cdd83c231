"""The inputs of the weighted NNI climb's tests -- shared by the CPU test, which asserts that they exercise what they are there for
(the kept-worse step of iqtree.cpp:2258, several NNIs in one step, the step cap), and the GPU test, which compares the engine with
the witness on them (tests/nni_snk_witness.py)."""
import numpy as np

from helpers import load_fixture
from nni_snk_witness import SnkNniWitness, SnkScorer


def tstv():
    c = np.full((4, 4), 2, dtype=np.uint32)
    np.fill_diagonal(c, 0)
    c[0, 2] = c[2, 0] = c[1, 3] = c[3, 1] = 1
    return c


def metric(S, seed):
    """symmetric and triangle-closed: Manhattan distances of random points"""
    pts = np.random.default_rng(seed).integers(0, 12, size=(S, 3))
    c = np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2).astype(np.uint32)
    c[c == 0] = 1
    np.fill_diagonal(c, 0)
    return c


def asym(S, seed):
    """i -> j and j -> i differ (upper triangle dearer); closed under the triangle repair the loader applies (parstree.cpp:74-80), so
    that engine, witness and oracle all see the matrix as given"""
    c = np.random.default_rng(seed).integers(1, 7, size=(S, S)).astype(np.int64)
    c[np.triu_indices(S, 1)] += 2
    np.fill_diagonal(c, 0)
    for k in range(S):
        c = np.minimum(c, c[:, k:k + 1] + c[k:k + 1, :])
    assert (c != c.T).any()
    return c.astype(np.uint32)


def cost_of(kind, S, seed=4):
    if kind == "tstv":
        return tstv()
    return metric(S, seed) if kind == "metric" else asym(S, seed)


# start: seed of mpboot_amd.trees.random_topology; root: 1 or "n" (the last taxon); steps: max_steps (the reference's MAXSTEPS is 50)
CASES = [
    dict(id="dna_clean-tstv", fx="dna_clean", cost="tstv", start=0, root=1, steps=50),
    dict(id="dna_ambig-asym-root-n", fx="dna_ambig", cost="asym", start=1, root="n", steps=50),
    dict(id="dna_dups-metric-weights", fx="dna_dups", cost="metric", start=2, root=1, steps=50),
    dict(id="aa-metric", fx="aa", cost="metric", start=0, root=1, steps=50),
    dict(id="dna_48-asym", fx="dna_48", cost="asym", start=0, root=1, steps=50),
    dict(id="dna_48-tstv-cap-3", fx="dna_48", cost="tstv", start=1, root="n", steps=3),
    dict(id="aa_40-asym-root-n", fx="aa_40", cost="asym", start=0, root="n", steps=50),
    dict(id="aa_40-metric", fx="aa_40", cost="metric", start=3, root=1, steps=50),
]


def setup(case):
    """-> (fixture, cost matrix, n, root taxon, start back[], scorer)"""
    from mpboot_amd import trees
    fx = load_fixture(case["fx"])
    n = fx["codes_np"].shape[0]
    cost = cost_of(case["cost"], fx["S"])
    root = n if case["root"] == "n" else 1
    back = trees.random_topology(n, np.random.default_rng(case["start"]))
    scorer = SnkScorer(fx["codes_np"], fx["weights_np"], cost, protein=fx["S"] == 20)
    return fx, cost, n, root, back, scorer


def witness(case, speednni, scorer=None, max_steps=None):
    fx, cost, n, root, back, sc = setup(case)
    w = SnkNniWitness(back, n, scorer or sc, root_taxon=root)
    w.result = w.optimize(speednni=speednni, max_steps=case["steps"] if max_steps is None else max_steps)
    return w
