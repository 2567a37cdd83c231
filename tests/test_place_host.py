"""The device-free part of taxon insertion (mpboot_amd/host/place_tree.hpp: the relaxed check of a backbone, the walk and branch
order, the first-minimum rule, the growth of the lists, my_random_shuffle, plain host costs) as a stand-alone program built with
-fsanitize=address,undefined, against tests/place_witness.py.  No GPU, nothing loaded into python: the program runs as a child
process and a sanitizer report fails the run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import place_witness as plw
from helpers import ROOT
from mpboot_amd.rng import Lcg64

SRC = os.path.join(ROOT, "mpboot_amd", "host", "place_host_main.cpp")
SIZES = (4, 5, 12, 33, 65)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("place_host") / "place_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _run(prog, *args):
    r = subprocess.run([prog, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def _write(path, n, first, nbr, root, query=(), tips=None):
    S, W = (0, 0) if tips is None else tips.shape[1:]
    head = np.array([n, S, W, len(first) - 1, root, len(query)], dtype=np.int32)
    with open(path, "wb") as f:
        for a in (head, np.asarray(first, dtype=np.int32), np.asarray(nbr, dtype=np.int32), np.asarray(query, dtype=np.int32)):
            f.write(a.tobytes())
        if tips is not None:
            f.write(np.ascontiguousarray(tips, dtype=np.uint32).tobytes())
    return path


def _rows(sets, S):
    """state-set masks [n][P] -> the engine's row layout [n][S][W], one bit per pattern, padding bits set in every row"""
    n, P = sets.shape
    W = (P + 31) // 32
    out = np.zeros((n, S, W), dtype=np.uint32)
    for s in range(S):
        bits = np.ones((n, 32 * W), dtype=np.uint64)
        bits[:, :P] = (sets >> s) & 1
        out[:, s, :] = (bits.reshape(n, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_walk_costs_first_minimum_and_growth(prog, tmp_path, n):
    rng = np.random.default_rng(n)
    p = str(tmp_path / "t.bin")
    P = 70
    codes = (1 << rng.integers(0, 4, size=(n, P))).astype(np.uint8)
    codes = np.where(rng.random((n, P)) < 0.1, rng.integers(1, 16, size=(n, P)), codes).astype(np.uint8)
    wit = plw.PlaceWitness(codes, np.ones(P, dtype=np.int64), 0)
    tips = _rows(plw.tip_sets(codes, 0), 4)
    for m in sorted({3, max(3, n // 2), n - 1}):
        present = rng.permutation(n)[:m] + 1
        first, nbr = plw.backbone(n, present, rng)
        rest = [t for t in range(1, n + 1) if t not in present.tolist()]
        for root in (int(present[0]), int(present[-1])):
            out = _run(prog, "check", _write(p, n, first, nbr, root))
            br = plw.walk(first, nbr, n, root)
            assert out[0] == "ok" and [int(x) for x in out[1].split()[1:]] == [v for ab in br for v in ab]
            # host costs: every query on every branch, the first minimum, the backbone's length
            out = _run(prog, "costs", _write(p, n, first, nbr, root, rest, tips))
            wbr, cost, length = wit.view_costs(first, nbr, rest, root)
            assert out[0] == "length %d" % length == "length %d" % wit.length(first, nbr, root)
            rows = [[int(x) for x in line.split()[2:]] for line in out if line.startswith("row ")]
            best = [int(line.split()[2]) for line in out if line.startswith("best ")]
            assert rows == cost.tolist() and best == [plw.first_min(r) for r in cost.tolist()]
            if n <= 12:
                assert (wit.costs(first, nbr, rest, root)[1] == cost).all()
        # growth: the remaining taxa attached one after the other at branches drawn from the walk
        f, nb, triples = list(first), list(nbr), []
        for t in rest:
            a, b = (lambda w: w[int(rng.integers(len(w)))])(plw.walk(f, nb, n, int(present[0])))
            triples += [t, a, b]
            f, nb = plw.grow(f, nb, n, t, a, b)
        out = _run(prog, "grow", _write(p, n, first, nbr, int(present[0]), triples))
        assert [int(x) for x in out[0].split()[1:]] == [int(x) for x in f] and [int(x) for x in out[1].split()[1:]] == nb
    assert _run(prog, "grow", _write(p, n, first, nbr, 1, [rest[0], 1, 1])) == ["no such branch"]


@pytest.mark.parametrize("n", SIZES)
def test_shuffle_is_my_random_shuffle(prog, n):
    for seed in (1, 77):
        g = Lcg64(seed)
        s0 = int(g.state)
        want = plw.shuffle(n, g)
        out = _run(prog, "shuffle", n, s0)
        assert [int(x) for x in out[0].split()[1:]] == want and sorted(want) == list(range(1, n + 1))
        assert int(out[1].split()[1]) == int(g.state)


def test_first_minimum(prog, tmp_path):
    p = str(tmp_path / "t.bin")
    for row in ([5, 3, 4, 3, 3], [2], [4, 4], [9, 8, 7], [1, 2, 1]):
        assert _run(prog, "firstmin", _write(p, 9, *plw.GOOD, 1, row)) == ["firstmin %d" % plw.first_min(row)]


def test_verdicts_on_malformed_lists(prog, tmp_path):
    p = str(tmp_path / "t.bin")
    assert _run(prog, "check", _write(p, 9, *plw.GOOD, 1))[0] == "ok"
    for name, (first, nbr, root, verdict) in plw.MALFORMED.items():
        out = _run(prog, "check", _write(p, 9, first, nbr, root))
        assert out[0].startswith(verdict + ": ") and plw.check(first, nbr, 9, root) == verdict, name
    # a query that sits in the backbone
    tips = np.full((9, 4, 1), 0xFFFFFFFF, dtype=np.uint32)
    assert _run(prog, "costs", _write(p, 9, *plw.GOOD, 1, [6, 3], tips)) == ["invalid: query 3"]
