"""The host-only part of the bootstrap summary (mpboot_amd/host/split_sets.hpp: the contract order, the greedy compatibility pass,
the neighbour lists built from the kept sets, and the host's own exact split count that resolves the device's overflow list) as a
stand-alone program built with -fsanitize=address,undefined, against the Python restatement of tests/splits_witness.py.  No GPU,
nothing loaded into python: the program runs as a child process and a sanitizer report fails the run.

tests/golden/splits/*.txt are tables of distinct splits in shuffled order: "n m total", then m rows "count word0 word1 ..." (hex)."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import splits_witness as sw
from helpers import ROOT
from mpboot_amd import trees

SRC = os.path.join(ROOT, "mpboot_amd", "host", "splits_host_main.cpp")
TABLES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "splits", "*.txt")))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("splits_host") / "splits_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _run(prog, mode, path, threshold):
    r = subprocess.run([prog, mode, path, repr(float(threshold))], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        k, *v = line.split()
        out[k] = v
    return out


def _ints(v):
    return [int(x) for x in v]


def _read_table(path):
    with open(path) as f:
        n, m, total = (int(x) for x in f.readline().split())
        rows = []
        for _ in range(m):
            tok = f.readline().split()
            rows.append((sw.words_set([int(x, 16) for x in tok[1:]]), int(tok[0])))
    return n, total, rows


def test_there_are_tables():
    assert len(TABLES) >= 4


@pytest.mark.parametrize("path", TABLES, ids=[os.path.basename(p)[:-4] for p in TABLES])
@pytest.mark.parametrize("threshold", (0.0, 0.5, 0.75))
def test_order_greedy_and_lists(prog, path, threshold):
    n, total, rows = _read_table(path)
    out = _run(prog, "tables", path, threshold)
    ordered = sw.contract_order(dict(rows), n)
    assert [rows[i] for i in _ints(out["order"])] == ordered
    kept = sw.greedy(ordered, total, threshold, n)
    assert [ordered[i] for i in _ints(out["kept"])] == kept
    first, nbr, sup = sw.build_lists(kept, n)
    assert (_ints(out["first"]), _ints(out["nbr"]), _ints(out["support"])) == (first, nbr, sup)
    # and the lists are that tree: its non-trivial splits are the kept sets
    below = sw.list_splits(_ints(out["first"]), _ints(out["nbr"]), n)
    assert {s for s in below.values() if len(s) < n - 1} == {s for s, _ in kept}
    if threshold >= 0.5:
        assert {s for s, _ in kept} == {s for s, c in rows if 2 * c > total and c > threshold * total}


def test_the_tables_cover_a_polytomy_a_majority_and_a_full_tree():
    shapes = set()
    for path in TABLES:
        n, total, rows = _read_table(path)
        k = len(sw.greedy(sw.contract_order(dict(rows), n), total, 0.5, n))
        shapes.add("star" if k == 0 else "full" if k == n - 3 else "partial")
    assert shapes == {"star", "full", "partial"}


@pytest.mark.parametrize("n", (4, 5, 31, 32, 33, 64, 65, 97))
def test_host_count_of_trees(prog, tmp_path, n):
    """the host's walk (the one k_split_keys mirrors) and its exact count, on trees: random ones, a caterpillar, a balanced one, one
    of weight 0 and weights above 1"""
    rng = np.random.default_rng(100 + n)
    backs = [trees.random_topology(n, rng) for _ in range(6)] + [sw.caterpillar(n), sw.balanced(n)]
    backs.append(backs[2].copy())
    weights = [1, 3, 2, 0, 1, 5, 1, 2, 4]
    path = str(tmp_path / "trees.bin")
    with open(path, "wb") as f:
        np.array([n, len(backs), 1], dtype=np.int32).tofile(f)
        np.asarray(backs, dtype=np.int32).tofile(f)
        np.asarray(weights, dtype=np.int32).tofile(f)
    out = _run(prog, "trees", path, 0.5)
    c, total = sw.counts(backs, weights)
    ordered = sw.contract_order(c, n)
    words = sw.words_of(n)
    bits = [int(x, 16) for x in out.get("bits", [])]
    got = [(sw.words_set(bits[i * words:(i + 1) * words]), k) for i, k in enumerate(_ints(out["count"]))]
    assert int(out["total"][0]) == total and int(out["n_distinct"][0]) == len(c)
    assert got == ordered
    # the supports of the first tree's clusters, by the inner node below each branch
    below = {}
    b0 = backs[0]

    def tips(rec):
        v = rec // 3
        if v <= n:
            return frozenset([v])
        s = tips(int(b0[trees.nxt(rec)])) | tips(int(b0[trees.nxt(trees.nxt(rec))]))
        below[v] = s
        return s

    tips(int(b0[3]))
    nodes, sup = _ints(out.get("target_node", [])), _ints(out.get("target_support", []))
    assert len(nodes) == n - 3 and sorted(nodes) == sorted(v for v, s in below.items() if len(s) < n - 1)
    assert sup == [c[below[v]] for v in nodes]
    kept = sw.greedy(ordered, total, 0.5, n)
    assert (_ints(out["first"]), _ints(out["nbr"]), _ints(out["support"])) == sw.build_lists(kept, n)


@pytest.mark.parametrize("kind", ("unlinked", "cycle", "cycle_caterpillar", "cycle_balanced"))
def test_a_broken_tree_is_refused(prog, tmp_path, kind):
    """... also records that link both ways everywhere and still are no tree: the walk is bounded by a tree's node counts"""
    n = 8 if kind == "unlinked" else 13
    b = trees.random_topology(n, np.random.default_rng(1))
    if kind == "unlinked":
        b[3 * (n + 2) + 1] = -1
    else:
        b = sw.cyclic_records({"cycle": b, "cycle_caterpillar": sw.caterpillar(n), "cycle_balanced": sw.balanced(n)}[kind], n)
        for v in range(1, 2 * n - 1):
            for s in range(1 if v <= n else 3):
                assert b[b[3 * v + s]] == 3 * v + s
    path = str(tmp_path / "bad.bin")
    with open(path, "wb") as f:
        np.array([n, 1, 0], dtype=np.int32).tofile(f)
        b.astype(np.int32).tofile(f)
    r = subprocess.run([prog, "trees", path, "0"], capture_output=True, text=True)
    assert r.returncode == 3 and "not a complete tree" in r.stderr
