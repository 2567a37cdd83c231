"""The IQ-TREE-level NNI entry point (integration/phylotree_shim.cpp: mpfitch_optimize_nni) through a stand-in tree driver
(tests/nni_shim_driver.cpp): the host's tree ends with the topology, slot order included, and the score of mpf_optimize_nni."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-in driver"
    exe = str(tmp_path_factory.mktemp("nni_shim") / "nni_shim_driver")
    lib = os.path.join(ROOT, "mpboot_amd")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "nni_shim_driver.cpp"),
                           os.path.join(ROOT, "integration", "phylotree_shim.cpp"), "-L" + lib, "-lmpfitch", "-Wl,-rpath," + lib])
    return exe


def _nei_table(back, n):
    return [[int(back[3 * (i + 1) + s]) // 3 - 1 for s in range(1 if i < n else 3)] for i in range(2 * n - 2)]


@pytest.mark.parametrize("name,alpha,dt", [("dna_ambig", "DNA", 0), ("aa", "AA", 1), ("dna_48", "DNA", 0)])
@pytest.mark.parametrize("speednni", [1, 0])
def test_dropin_climb_equals_the_engine(driver, name, alpha, dt, speednni):
    from mpboot_amd import engine, trees
    from oracle import iqtree_fitch
    fx = load_fixture(name)
    states = iqtree_fitch.convert_states(fx["rows"], alpha)
    n, P = states.shape
    freq = np.asarray(fx["weights"], dtype=np.int32)
    for seed in (0, 1):
        back = trees.random_topology(n, np.random.default_rng(seed))
        root = seed * (n - 1)                                   # leaf id 0, then the last taxon
        lines = [f"{n} {P} {dt}", " ".join(map(str, freq))]
        lines += [" ".join(str(int(v)) for v in row) for row in states]
        lines += [f"{len(r)} " + " ".join(map(str, r)) for r in _nei_table(back, n)]
        lines.append(f"{root} {speednni}")
        res = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        out = res.stdout.splitlines()
        head = out[0].split()
        got_score, got_count, got_steps = int(head[1]), int(head[3]), int(head[5])
        got_nei = [[int(x) for x in ln.split()[1:]] for ln in out[1:]]

        codes = engine.encode_iqtree_states(states, dt)
        eng = engine.FitchEngine(codes, freq, datatype=dt, keep_all=True)
        eng.set_tree(back)
        want = eng.optimize_nni(root + 1, bool(speednni))
        assert (got_score, got_count, got_steps) == want
        assert got_nei == _nei_table(eng.get_tree(), n)
        assert got_score == eng.score_tree(eng.get_tree())
