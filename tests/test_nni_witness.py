"""CPU checks of the NNI climb's witness (tests/nni_witness.py): its std::sort port against libstdc++, its move lengths against
a second scorer, and the NNI optimality of where it ends."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import load_fixture
from nni_witness import NniWitness, std_sort
from oracle import iqtree_fitch, pyoracle as po

SORT_SRC = r"""
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>
int main()
{
  int t;
  if (std::scanf("%d", &t) != 1) return 1;
  while (t--) {
    int n;
    if (std::scanf("%d", &n) != 1) return 1;
    std::vector<std::pair<int, int>> a(n);
    for (int i = 0; i < n; i++) { if (std::scanf("%d", &a[i].first) != 1) return 1; a[i].second = i; }
    std::sort(a.begin(), a.end(), [](const std::pair<int, int> &x, const std::pair<int, int> &y) { return x.first < y.first; });
    for (int i = 0; i < n; i++) std::printf("%d ", a[i].second);
    std::printf("\n");
  }
  return 0;
}
"""


def test_std_sort_port_is_the_libstdcxx_permutation(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to pin the std::sort port"
    src = tmp_path / "sort.cpp"
    src.write_text(SORT_SRC)
    exe = tmp_path / "sort"
    subprocess.check_call([gxx, "-O1", "-std=c++17", str(src), "-o", str(exe)])
    rng = np.random.default_rng(11)
    cases = []
    for n in list(range(0, 40)) + list(rng.integers(40, 301, size=260)):
        k = int(rng.choice([1, 2, 3, 5, max(1, n // 8), max(1, n // 2), n + 1]))
        cases.append([int(v) for v in rng.integers(0, k, size=int(n))])
    cases.append(list(range(300, 0, -1)))
    cases.append([7] * 300)
    feed = f"{len(cases)}\n" + "".join(f"{len(c)} {' '.join(map(str, c))}\n" for c in cases)
    out = subprocess.run([str(exe)], input=feed, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for c, line in zip(cases, out):
        want = [int(x) for x in line.split()]
        got = [i for _v, i in std_sort([(v, i) for i, v in enumerate(c)], lambda a, b: a[0] < b[0])]
        assert got == want, (len(c), c[:20])


def _start_trees(fx, seeds=(1, 2)):
    o = po.Oracle(fx["codes_np"], fx["weights_np"], datatype=fx["datatype"])
    for s in seeds:
        o.stepwise(s)
        yield o, o.get_tree()


@pytest.mark.parametrize("name,alpha,ns", [("dna_clean", "DNA", 4), ("dna_ambig", "DNA", 4), ("aa", "AA", 20)])
def test_witness_move_lengths_match_a_second_scorer(name, alpha, ns):
    fx = load_fixture(name)
    states = iqtree_fitch.convert_states(fx["rows"], alpha)
    n = fx["codes_np"].shape[0]
    for o, back in _start_trees(fx):
        w = NniWitness(back, n, lambda b: o.score_tree(b))
        order = w.full_order()
        assert len(order) == n - 3
        for v1, v2 in order:
            l0, l1, m0, m1 = w.score_branch(v1, v2)
            for ln, mv in ((l0, m0), (l1, m1)):
                w.swap(mv, log=False)
                s, _ = iqtree_fitch.compute_parsimony(states, fx["weights"], w.back, ns)
                w.swap(mv, log=False)
                assert s == ln, (name, v1, v2, mv)
        assert (w.back == back).all()


@pytest.mark.parametrize("name", ["dna_clean", "dna_48", "aa_40"])
def test_witness_without_speednni_ends_nni_optimal(name):
    fx = load_fixture(name)
    n = fx["codes_np"].shape[0]
    for o, back in _start_trees(fx):
        w = NniWitness(back, n, lambda b: o.score_tree(b))
        length, count, steps = w.optimize(speednni=False)
        assert length == o.score_tree(w.back)
        assert steps <= 51 and count >= 0
        for _v1, _v2, l0, l1 in w.scores():
            assert min(l0, l1) >= length
        # the log replayed on the start tree gives the final tree
        r = NniWitness(back, n, None)
        for mv in w.log:
            r.swap(mv)
        assert (r.back == w.back).all()
