"""The host-only part of the split products on trees given as neighbour lists (mpboot_amd/host/split_sets.hpp: lists_ok,
walk_clusters_lists, count_splits and host_rf on mixed sets) as a stand-alone program built with -fsanitize=address,undefined,
against the Python restatement of tests/split_lists_witness.py.  No GPU, nothing loaded into python: the program runs as a child
process and a sanitizer report fails the run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import split_lists_witness as lw
import splits_witness as sw
from helpers import ROOT
from mpboot_amd import trees

SRC = os.path.join(ROOT, "mpboot_amd", "host", "split_lists_host_main.cpp")
ALL, ADJ, TWO = 0, 1, 2
SIZES = (4, 5, 12, 33, 65)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("split_lists_host") / "split_lists_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _run(prog, *args):
    r = subprocess.run([prog, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


write_sets = lw.write_sets


def _set_order(items):
    return [items[i] for i in lw.as_engine_args(list(items))[2]]


def _shapes(n):
    """record trees, their contractions, and the edge shapes: the star, a caterpillar contracted to one deep chain, a hub in the middle,
    a fully resolved tree as lists"""
    rng = np.random.default_rng(100 + n)
    backs = sw.related_trees(n, 4, 7 + n, 3)
    items = [backs[0], lw.star(n), trees.back_to_lists(backs[1], n), backs[1]]
    if n >= 5:
        items.append(lw.middle_hub(n))
        cat = sw.caterpillar(n)
        br = lw.inner_branches(cat, n)
        items.append(trees.collapse_branches(cat, n, br[::2]))       # every second branch of the chain: still n deep
        items.append(lw.collapse(backs[2], n, 1, rng))
        items.append(lw.collapse(backs[3], n, (n - 3) // 2, rng))
        items.append(lw.collapse(backs[3], n, n - 3, rng))            # everything contracted: the star again
    return items


@pytest.mark.parametrize("n", SIZES)
def test_walk_against_the_witness(prog, tmp_path, n):
    items = _shapes(n)
    lists = [t for t in items if lw.is_lists(t)]
    out = _run(prog, "walk", write_sets(str(tmp_path / "t.bin"), n, ALL, items))
    assert not any(line.endswith("bad") for line in out)
    for k, (first, nbr) in enumerate(lists):
        tag = "list %d " % k
        mine = [line[len(tag):].split() for line in out if line.startswith(tag)]
        order = next([int(x) for x in r[1:]] for r in mine if r[0] == "order")
        pos = next([int(x) for x in r[1:]] for r in mine if r[0] == "pos")
        cl = [tuple(int(x) for x in r[1:]) for r in mine if r[0] == "cluster"]
        below = sw.list_splits(first, nbr, n)
        walk = lw.branch_walk(first, nbr, n)
        # tips in the order the branch walk meets them; tip 1 outside every interval
        assert order == [b for _, b in walk if b <= n] and sorted(order) == list(range(2, n + 1))
        assert pos[0] == n - 1 and all(pos[t - 1] == i for i, t in enumerate(order))
        # one cluster per inner node but the first, in the order the walk meets them, each the interval of the tips below it
        assert [c[2] for c in cl] == [b for _, b in walk if b > n][1:] and len(cl) == len(first) - 2
        for lo, hi, node in cl:
            assert frozenset(order[lo:hi]) == below[node]
        assert frozenset(frozenset(order[lo:hi]) for lo, hi, _ in cl) == lw.splits_of((first, nbr), n)
        assert len(lw.splits_of((first, nbr), n)) == len(first) - 2


@pytest.mark.parametrize("n", SIZES)
def test_host_rf_and_counts_against_the_witness(prog, tmp_path, n):
    items = _shapes(n)
    so = _set_order(items)
    sets = lw.split_sets(so, n)
    p = str(tmp_path / "t.bin")

    def rf(*a, **k):
        line = next(x for x in _run(prog, "rf", write_sets(p, n, *a, **k)) if x.startswith("rf"))
        return [int(x) for x in line.split()[1:]]

    full = lw.all_pairs(sets)
    assert rf(ALL, items) == full.reshape(-1).tolist()
    assert rf(ADJ, items) == lw.adjacent(sets).tolist()
    a, b = items[:3], items[2:]
    assert rf(TWO, a, b) == lw.two_sets(lw.split_sets(_set_order(a), n), lw.split_sets(_set_order(b), n)).reshape(-1).tolist()
    # a fully resolved tree as lists is its record form: distance 0 (items[2] and items[3]), n - 3 from the star
    i1, i2, i3 = ([k for k, t in enumerate(so) if t is items[i]][0] for i in (1, 2, 3))
    assert full[i2, i3] == 0 and full[i1, i3] == n - 3
    # lists alone, and one tree
    only = [t for t in items if lw.is_lists(t)]
    assert rf(ALL, only) == lw.all_pairs(lw.split_sets(only, n)).reshape(-1).tolist()
    assert rf(ALL, only[:1]) == [0] and rf(ADJ, only[:1]) == []
    # weighted counts, weight 0 on one tree and a star of weight > 0
    w = [(3 * i + 1) % 5 for i in range(len(items))]
    w[1], w[0] = 4, 0
    out = _run(prog, "counts", write_sets(p, n, ALL, items, weights=w))
    words, cnt, total = lw.ordered_table(lw.split_sets(items, n), w, n)
    assert out[0] == "total %d" % total
    got = [line.split()[1:] for line in out[1:]]
    assert [int(g[0]) for g in got] == cnt
    assert [tuple(int(x, 16) for x in g[1:]) for g in got] == words


_broken, BROKEN = lw.broken_lists, lw.BROKEN


@pytest.mark.parametrize("kind", BROKEN)
def test_lists_ok_refuses(prog, tmp_path, kind):
    n = 9
    good = _broken("good")
    out = _run(prog, "check", write_sets(str(tmp_path / "t.bin"), n, ALL, [good, _broken(kind), good]))
    assert out[0] == "list 0 ok" and out[2] == "list 2 ok" and out[1].startswith("list 1 bad: ")
    # ... and the calls built on it name the tree (the record tree in front counts)
    rec = sw.caterpillar(n)
    for cmd in ("rf", "counts"):
        r = subprocess.run([prog, cmd, write_sets(str(tmp_path / "u.bin"), n, ALL, [rec, good, _broken(kind)])], capture_output=True, text=True)
        assert r.returncode == 3 and "tree 2 is not a complete tree" in r.stderr
    # the walk alone is bounded too: it ends, with or without a refusal, and the sanitizers stay quiet
    _run(prog, "walk", write_sets(str(tmp_path / "t.bin"), n, ALL, [_broken(kind)]))


def test_sizes_that_are_no_tree(prog, tmp_path):
    n = 9
    good = _broken("good")
    out = _run(prog, "check", write_sets(str(tmp_path / "t.bin"), n, ALL, [good, (np.zeros(9, dtype=np.int32), np.zeros(0, dtype=np.int32))]))
    assert out == ["list 0 ok", "list 1 bad: n_inner or first[] are not those of a tree"]


def test_three_taxa(prog, tmp_path):
    """one tree shape, the star: no split, every distance 0"""
    t3 = trees.newick_to_back("(1,2,3);", ["1", "2", "3"])
    items = [t3, lw.star(3), lw.star(3)]
    p = str(tmp_path / "t.bin")
    assert _run(prog, "rf", write_sets(p, 3, ALL, items))[0] == "rf" + " 0" * 9
    assert _run(prog, "rf", write_sets(p, 3, ADJ, items))[0] == "rf 0 0"
    assert _run(prog, "rf", write_sets(p, 3, TWO, items[:1], items[1:]))[0] == "rf 0 0"
    assert _run(prog, "counts", write_sets(p, 3, ALL, items)) == ["total 3"]
    assert _run(prog, "walk", write_sets(p, 3, ALL, items[1:2])) == ["list 0 order 2 3", "list 0 pos 2 0 1"]
