"""The host-only part of the Robinson-Foulds distances (mpboot_amd/host/split_sets.hpp: the plain host RF, the column numbering of
overflow groups, the chunk plan) as a stand-alone program built with -fsanitize=address,undefined, against the Python restatement
of tests/rf_witness.py.  No GPU, nothing loaded into python: the program runs as a child process and a sanitizer report fails
the run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rf_witness as rw
import splits_witness as sw
from helpers import ROOT
from mpboot_amd import trees

SRC = os.path.join(ROOT, "mpboot_amd", "host", "rf_host_main.cpp")
ALL, ADJ, TWO = 0, 1, 2


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("rf_host") / "rf_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _run(prog, *args):
    r = subprocess.run([prog, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        k, *v = line.split()
        out[k] = [int(x) if k != "ms_rf" else float(x) for x in v]
    return out


def _write(path, n, mode, backs, backs2=()):
    with open(path, "wb") as f:
        np.array([n, mode, len(backs), len(backs2)], dtype=np.int32).tofile(f)
        np.asarray(backs, dtype=np.int32).tofile(f)
        if len(backs2):
            np.asarray(backs2, dtype=np.int32).tofile(f)
    return path


def _sets():
    rng = np.random.default_rng(61)
    return {"random12_n33": (33, [trees.random_topology(33, rng) for _ in range(12)]),
            "related40_n40": (40, sw.related_trees(40, 40, 21, 3))}


SETS = _sets()


@pytest.mark.parametrize("name", sorted(SETS))
def test_host_rf_against_the_witness(prog, tmp_path, name):
    n, backs = SETS[name]
    p = str(tmp_path / "t.bin")
    full = rw.all_pairs(backs)
    assert _run(prog, "rf", _write(p, n, ALL, backs))["rf"] == full.reshape(-1).tolist()
    assert _run(prog, "rf", _write(p, n, ADJ, backs))["rf"] == rw.adjacent(backs).tolist()
    h = len(backs) // 3
    a, b = backs[:h + 2], backs[h:]                      # two sets of different sizes with two trees in both
    assert _run(prog, "rf", _write(p, n, TWO, a, b))["rf"] == rw.two_sets(a, b).reshape(-1).tolist()
    assert (full == full.T).all() and (np.diag(full) == 0).all()
    if name.startswith("related"):
        assert 0 < full.max() < 2 * (n - 3)              # the trees share splits, and differ
    # one tree: the single 0, and no adjacent pair
    assert _run(prog, "rf", _write(p, n, ALL, backs[:1]))["rf"] == [0]
    assert _run(prog, "rf", _write(p, n, ADJ, backs[:1]))["rf"] == []


def test_overflow_columns(prog, tmp_path):
    """two groups that collide (sets A, B: three and two members), two sets that stand alone: distinct groups get distinct columns
    from first_col on, single-member groups none"""
    A, B, X, Y = ("00000006", "00000001"), ("00000018", "00000000"), ("00000060", "00000001"), ("00000006", "00000000")
    rows = [A, X, B, A, B, Y, A]
    path = str(tmp_path / "groups.txt")
    with open(path, "w") as f:
        f.write("2 %d 10\n" % len(rows))
        for r in rows:
            f.write(" ".join(r) + "\n")
    out = _run(prog, "groups", path)
    assert out["col"] == [10, -1, 11, 10, 11, -1, 10] and out["n_columns"] == [2]
    with open(path, "w") as f:
        f.write("2 0 7\n")
    out = _run(prog, "groups", path)
    assert out["col"] == [] and out["n_columns"] == [0]


@pytest.mark.parametrize("columns,rows,forced,budget", [(0, 64, 0, 1 << 20), (1, 64, 0, 1 << 20), (65, 64, 32, 1 << 20), (65, 64, 64, 1 << 20),
                                                        (200, 128, 33, 1 << 20), (5000, 1024, 0, 1 << 19), (5000, 1024, 0, 1 << 10),
                                                        (96, 64, 32, 1 << 20), (4097, 192, 0, 256 << 20)])
def test_chunk_plan(prog, columns, rows, forced, budget):
    k_step = 32
    out = _run(prog, "plan", columns, rows, forced, budget, k_step)
    c0, c1 = out["c0"], out["c1"]
    assert len(c0) == len(c1)
    if columns == 0:
        assert c0 == []
        return
    # every column once, in order
    assert c0[0] == 0 and c1[-1] == columns and c0[1:] == c1[:-1] and all(a < b for a, b in zip(c0, c1))
    sizes = [b - a for a, b in zip(c0, c1)]
    assert all(s % 32 == 0 for s in sizes[:-1]) and len(set(sizes[:-1])) <= 1 and sizes[-1] <= max(sizes)
    if forced:
        per = (forced + 31) // 32 * 32
        assert all(s == per for s in sizes[:-1]) and len(sizes) == -(-columns // per)
    else:
        # rows x padded words of every chunk within the budget, unless a chunk is already as narrow as the K step allows
        for s in sizes:
            words = -(-(-(-s // 32)) // k_step) * k_step
            assert rows * words * 4 <= budget or words == k_step
        # and no narrower than needed: one more K step would not have fitted
        if len(sizes) > 1:
            words = sizes[0] // 32
            assert words % k_step == 0 and (rows * (words + k_step) * 4 > budget or words == k_step)


@pytest.mark.parametrize("kind", ("unlinked", "cycle", "cycle_second_set"))
def test_a_broken_tree_is_refused(prog, tmp_path, kind):
    n = 13
    rng = np.random.default_rng(1)
    good = [trees.random_topology(n, rng) for _ in range(3)]
    b = good[1].copy()
    if kind == "unlinked":
        b[3 * (n + 2) + 1] = -1
    else:
        b = sw.cyclic_records(b, n)
    if kind == "cycle_second_set":
        path, want = _write(str(tmp_path / "bad.bin"), n, TWO, good, [good[0], b]), "tree 4 "
    else:
        path, want = _write(str(tmp_path / "bad.bin"), n, ALL, [good[0], b, good[2]]), "tree 1 "
    r = subprocess.run([prog, "rf", path], capture_output=True, text=True)
    assert r.returncode == 3 and "not a complete tree" in r.stderr and want in r.stderr
