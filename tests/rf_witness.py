"""Python restatement of the Robinson-Foulds distance, for the tests of mpf_rf_distances and of the host-only program: the number
of non-trivial splits in one tree and not in the other, from trees.splits (frozensets), and the three result layouts of
MTreeSet::computeRFDist built from it.  Written independently of mpboot_amd/host/split_sets.hpp: sets are Python frozensets here,
never words."""
import numpy as np

from mpboot_amd import trees


def split_sets(backs):
    """the split set of every tree, computed once"""
    return [frozenset(trees.splits(np.asarray(b))) for b in backs]


def rf(a, b):
    return len(trees.splits(np.asarray(a)) ^ trees.splits(np.asarray(b)))


def all_pairs(backs):
    s = split_sets(backs)
    out = np.zeros((len(s), len(s)), dtype=np.int32)
    for i in range(len(s)):
        for j in range(i + 1, len(s)):                  # a symmetric difference: one half computed, the other its mirror
            out[i, j] = out[j, i] = len(s[i] ^ s[j])
    return out


def adjacent(backs):
    s = split_sets(backs)
    return np.array([len(s[i] ^ s[i + 1]) for i in range(len(s) - 1)], dtype=np.int32)


def two_sets(backs, backs2):
    s, s2 = split_sets(backs), split_sets(backs2)
    return np.array([[len(x ^ y) for y in s2] for x in s], dtype=np.int32).reshape(len(s), len(s2))
