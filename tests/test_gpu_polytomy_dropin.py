"""A multifurcating tree at the IQ-TREE-level entry points (integration/phylotree_shim.cpp) through a stand-in tree driver
(tests/polytomy_shim_driver.cpp): with the optional hook table installed, computeParsimony() returns the witness's length and
_pattern_pars and mpfitch_fix_negative_branch rewrites every branch with the length the witness's count gives; without it the old
refusal stays."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nni_snk_cases as cases
import polytomy_witness as pw
from helpers import ROOT, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-in driver"
    exe = str(tmp_path_factory.mktemp("polytomy_shim") / "polytomy_shim_driver")
    lib = os.path.join(ROOT, "mpboot_amd")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "polytomy_shim_driver.cpp"),
                           os.path.join(ROOT, "integration", "phylotree_shim.cpp"), "-L" + lib, "-lmpfitch", "-Wl,-rpath," + lib])
    return exe


def _host_tree(first, nbr, n, inner_ids):
    """the lists as a host holds them: leaf ids 0 .. n - 1, inner node i under the id inner_ids[i]; -> {id: [neighbour ids]}"""
    hid = lambda v: v - 1 if v <= n else inner_ids[v - n - 1]
    nei = {hid(n + 1 + i): [hid(u) for u in pw.neighbours(first, nbr, n, n + 1 + i)] for i in range(len(first) - 1)}
    for v, lst in list(nei.items()):
        for u in lst:
            if u < n:
                nei[u] = [v]
    return nei


def _run(driver, states, freq, dt, nei, root, n_sites, force, parstree, cost, poly_hooks, lens):
    n, P = states.shape
    ids = sorted(nei)
    lines = [f"{n} {P} {dt}", " ".join(map(str, freq))]
    lines += [" ".join(str(int(v)) for v in row) for row in states]
    lines.append(str(len(ids)))
    lines += [f"{i} {len(nei[i])} " + " ".join(map(str, nei[i])) for i in ids]
    lines.append(f"{root} {n_sites} {force} {parstree} {0 if cost is None else 1} {poly_hooks}")
    if cost is not None:
        lines.append(" ".join(str(int(c)) for c in np.asarray(cost).ravel()))
    lines += [" ".join(repr(float(lens[(i, o)])) for o in nei[i]) for i in ids]
    res = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        return res, None
    out = res.stdout.splitlines()
    got = {}
    for i, ln in zip(ids, out[3:]):
        for o, v in zip(nei[i], ln.split()[1:]):
            got[(i, o)] = float(v)
    return res, (int(out[0].split()[1]), [int(x) for x in out[1].split()[1:]], int(out[2].split()[1]), got)


def _ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


@pytest.mark.parametrize("name,alpha,dt,weighted", [("dna_ambig", "DNA", 0, False), ("aa", "AA", 1, False), ("dna_ambig", "DNA", 0, True)])
def test_with_the_hooks_a_multifurcating_tree_is_served(driver, name, alpha, dt, weighted):
    from mpboot_amd import engine, trees
    from oracle import iqtree_fitch
    fx = load_fixture(name)
    states = iqtree_fitch.convert_states(fx["rows"], alpha)
    n, P = states.shape
    freq = np.asarray(fx["weights"], dtype=np.int32)
    codes = engine.encode_iqtree_states(states, dt)
    cost = cases.cost_of("asym", 4) if weighted else None
    wit = pw.PolyWitness(codes, freq, dt, cost=cost)
    for seed in (0, 1):
        rng = np.random.default_rng(seed)
        first, nbr = pw.random_collapse(trees.random_topology(n, rng), n, rng, 0.5)
        k = len(first) - 1
        assert k < n - 2 and int(np.diff(first).max()) > 3
        inner_ids = [n + 2 * i + seed for i in range(k)]         # (ids with gaps: the shim renumbers)
        nei = _host_tree(first, nbr, n, inner_ids)
        root = seed * (n - 1)
        hid = lambda v: v - 1 if v <= n else inner_ids[v - n - 1]
        lens = {(i, o): -1.0 if (i + o) % 3 else 0.25 for i in nei for o in nei[i]}
        want_len, want_ptn = wit.parsimony(first, nbr, root + 1)
        order, subst = wit.substitutions(first, nbr, root + 1)
        n_sites = 4 * int(subst.max()) if weighted else int(freq.sum())
        want_bl = pw.branch_lengths(subst, n_sites, wit.S)
        for force in (1, 0):
            res, out = _run(driver, states, freq, dt, nei, root, n_sites, force, -1, cost, 1, lens)
            assert res.returncode == 0, res.stderr
            score, ptn, fixed, got = out
            assert score == want_len and ptn == want_ptn.tolist()
            assert fixed == (n + k - 1 if force else sum(1 for v in lens.values() if v < 0) // 2)
            for (v1, v2), bl in zip(order, want_bl):
                a, b = hid(v1), hid(v2)
                assert got[(a, b)] == got[(b, a)]                 # both directions set
                if force or lens[(a, b)] < 0:
                    assert _ulps(got[(a, b)], bl) <= 4
                else:
                    assert got[(a, b)] == lens[(a, b)]


def test_a_resolved_tree_takes_the_old_path_with_the_hooks_installed(driver):
    from mpboot_amd import engine, trees
    from oracle import iqtree_fitch
    fx = load_fixture("dna_ambig")
    states = iqtree_fitch.convert_states(fx["rows"], "DNA")
    n, P = states.shape
    freq = np.asarray(fx["weights"], dtype=np.int32)
    codes = engine.encode_iqtree_states(states, 0)
    back = trees.random_topology(n, np.random.default_rng(4))
    first, nbr = trees.collapse_branches(back, n, ())
    nei = _host_tree(first, nbr, n, list(range(n, 2 * n - 2)))
    lens = {(i, o): -1.0 for i in nei for o in nei[i]}
    eng = engine.FitchEngine(codes, freq, datatype=0, keep_all=True)
    eng.set_tree(back)
    a, b, want = eng.branch_lengths(int(freq.sum()), 1)
    outs = []
    for hooks in (0, 1):
        res, out = _run(driver, states, freq, 0, nei, 0, int(freq.sum()), 1, -1, None, hooks, lens)
        assert res.returncode == 0, res.stderr
        outs.append(out)
        assert out[0] == eng.score_tree(back) and out[2] == 2 * n - 3
        assert all(out[3][(int(x) - 1, int(y) - 1)] == float(w) for x, y, w in zip(a, b, want))
    assert outs[0] == outs[1]


def test_without_the_hooks_the_old_refusal(driver):
    from mpboot_amd import engine, trees
    from oracle import iqtree_fitch
    fx = load_fixture("dna_ambig")
    states = iqtree_fitch.convert_states(fx["rows"], "DNA")
    n, P = states.shape
    freq = np.asarray(fx["weights"], dtype=np.int32)
    rng = np.random.default_rng(0)
    first, nbr = pw.random_collapse(trees.random_topology(n, rng), n, rng, 0.5)
    nei = _host_tree(first, nbr, n, list(range(n, n + len(first) - 1)))
    lens = {(i, o): -1.0 for i in nei for o in nei[i]}
    res, out = _run(driver, states, freq, 0, nei, 0, int(freq.sum()), 1, -1, None, 0, lens)
    assert res.returncode != 0 and out is None
    # marshal_tree's exit: a node without its three neighbours, or one whose neighbour lists it beyond the third place
    assert "mpfitch phylotree shim" in res.stderr
    assert "multifurcating or rooted tree?" in res.stderr or "are not mutual neighbours" in res.stderr
