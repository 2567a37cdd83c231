"""The IQ-TREE-level branch-length entry point (integration/phylotree_shim.cpp: mpfitch_fix_negative_branch) through a stand-in
tree driver (tests/brlen_shim_driver.cpp): the host's tree ends with the lengths PhyloTree::fixNegativeBranch (reference
phylotree.cpp:3597-3633) leaves, on both directions of every branch, and the count of rewritten branches it returns."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nni_snk_cases as cases
from helpers import ROOT, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-in driver"
    exe = str(tmp_path_factory.mktemp("brlen_shim") / "brlen_shim_driver")
    lib = os.path.join(ROOT, "mpboot_amd")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "brlen_shim_driver.cpp"),
                           os.path.join(ROOT, "integration", "phylotree_shim.cpp"), "-L" + lib, "-lmpfitch", "-Wl,-rpath," + lib])
    return exe


def _nei_table(back, n):
    return [[int(back[3 * (i + 1) + s]) // 3 - 1 for s in range(1 if i < n else 3)] for i in range(2 * n - 2)]


def _run(driver, states, freq, dt, back, root, n_sites, force, parstree, cost, lens):
    """lens: {(id1, id2): length} for both directions -> (fixed, {(id1, id2): length})"""
    n, P = states.shape
    nei = _nei_table(back, n)
    lines = [f"{n} {P} {dt}", " ".join(map(str, freq))]
    lines += [" ".join(str(int(v)) for v in row) for row in states]
    lines += [f"{len(r)} " + " ".join(map(str, r)) for r in nei]
    lines.append(f"{root} {n_sites} {force} {parstree} {0 if cost is None else 1}")
    if cost is not None:
        lines.append(" ".join(str(int(c)) for c in np.asarray(cost).ravel()))
    lines += [" ".join(repr(float(lens[(i, o)])) for o in r) for i, r in enumerate(nei)]
    res = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    out = res.stdout.splitlines()
    fixed = int(out[0].split()[1])
    got = {}
    for i, (r, ln) in enumerate(zip(nei, out[1:])):
        for o, v in zip(r, ln.split()[1:]):
            got[(i, o)] = float(v)
    return fixed, got


def _expect(a, b, want_len, lens, force):
    """fixNegativeBranch over the branches (a[i], b[i]) in order: -> (fixed, lengths)"""
    out = dict(lens)
    fixed = 0
    for x, y, w in zip(a, b, want_len):
        x, y = int(x) - 1, int(y) - 1
        cur = out[(x, y)]
        if cur < 0.0 or force:
            cur = float(w)
            out[(x, y)] = out[(y, x)] = cur
            fixed += 1
        if cur <= 0.0:
            out[(x, y)] = out[(y, x)] = 1e-6
    return fixed, out


def _start_lengths(back, n, rng):
    """a third negative, a few zero, the rest positive -- the same on both directions, as a tree read from a file has them"""
    lens = {}
    for i, r in enumerate(_nei_table(back, n)):
        for o in r:
            if (o, i) in lens:
                lens[(i, o)] = lens[(o, i)]
            else:
                u = rng.random()
                lens[(i, o)] = -0.5 if u < 0.33 else (0.0 if u < 0.45 else float(rng.random()) + 0.01)
    return lens


@pytest.mark.parametrize("name,alpha,dt", [("dna_ambig", "DNA", 0), ("aa", "AA", 1)])
def test_dropin_lengths_equal_the_engine(driver, name, alpha, dt):
    from mpboot_amd import engine, trees
    from oracle import iqtree_fitch
    fx = load_fixture(name)
    states = iqtree_fitch.convert_states(fx["rows"], alpha)
    n, P = states.shape
    freq = np.asarray(fx["weights"], dtype=np.int32)
    n_sites = int(freq.sum())
    codes = engine.encode_iqtree_states(states, dt)
    eng = engine.FitchEngine(codes, freq, datatype=dt, keep_all=True)
    for seed in (0, 1):
        rng = np.random.default_rng(seed)
        back = trees.random_topology(n, rng)
        root = seed * (n - 1)                                   # leaf id 0, then the last taxon
        lens = _start_lengths(back, n, rng)
        assert any(v < 0 for v in lens.values()) and any(v == 0 for v in lens.values())
        eng.set_tree(back)
        a, b, want = eng.branch_lengths(n_sites, root + 1)
        for force in (1, 0):
            fixed, got = _run(driver, states, freq, dt, back, root, n_sites, force, -1, None, lens)
            want_fixed, want_lens = _expect(a, b, want, lens, force)
            assert fixed == want_fixed
            assert fixed == (2 * n - 3 if force else sum(1 for v in lens.values() if v < 0) // 2)
            assert got == want_lens
            assert all(got[(x, y)] == got[(y, x)] and got[(x, y)] >= 1e-6 for (x, y) in got)      # both directions set; zeros floored


def test_dropin_parstree_rules(driver):
    """a tree with a cost matrix takes ParsTree's rule on the weighted engine (every branch from the tree's length rooted there); a
    unit-cost ParsTree takes it on the Fitch engine, through the is_parstree hook and through a unit matrix alike"""
    from mpboot_amd import engine, trees
    from oracle import iqtree_fitch
    fx = load_fixture("dna_ambig")
    states = iqtree_fitch.convert_states(fx["rows"], "DNA")
    n, P = states.shape
    freq = np.asarray(fx["weights"], dtype=np.int32)
    codes = engine.encode_iqtree_states(states, 0)
    back = trees.random_topology(n, np.random.default_rng(3))
    lens = {k: -1.0 for k in _start_lengths(back, n, np.random.default_rng(3))}
    root = n - 1
    # (N large enough that x > 0 for a whole tree length)
    cost = cases.cost_of("asym", 4)
    snk = engine.FitchEngine(codes, freq, datatype=0, keep_all=True, cost=cost)
    snk.set_tree(back)
    n_sites = 4 * int(snk.branch_substitutions(root + 1)[2].max())
    a, b, want = snk.branch_lengths(n_sites, root + 1)
    assert len(set(want.tolist())) > 1                          # the orientation shows
    fixed, got = _run(driver, states, freq, 0, back, root, n_sites, 0, -1, cost, lens)
    assert fixed == 2 * n - 3 and got == _expect(a, b, want, lens, 0)[1]
    fit = engine.FitchEngine(codes, freq, datatype=0, keep_all=True)
    fit.set_tree(back)
    a, b, want = fit.branch_lengths(n_sites, root + 1, unit_cost_parstree=True)
    assert len(set(want.tolist())) == 1
    assert (fit.branch_lengths(n_sites, root + 1)[2] != want).any()
    unit = 1 - np.eye(4, dtype=np.uint32)
    for parstree, matrix in ((1, None), (-1, unit), (1, unit)):
        fixed, got = _run(driver, states, freq, 0, back, root, n_sites, 1, parstree, matrix, lens)
        assert fixed == 2 * n - 3 and got == _expect(a, b, want, lens, 1)[1]
