"""The bootstrap-summary entry points are part of the C-ABI: exported, declared, bound, and the ABI number stays 8.  No GPU."""
import ctypes
import os

from helpers import ROOT

NAMES = ("mpf_split_counts", "mpf_split_support", "mpf_consensus_tree", "mpf_ufboot_summarize", "mpf_ufboot_summary_trees")


def _lib():
    import __graft_entry__ as g
    path = os.path.join(ROOT, "mpboot_amd", "libmpfitch.so")
    if not os.path.exists(path):
        g.build()
    return ctypes.CDLL(path)


def test_the_symbols_are_exported_and_the_abi_is_8():
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.mpf_abi_version.restype = ctypes.c_int
    assert lib.mpf_abi_version() == 8


def test_header_and_binding_name_them():
    from mpboot_amd import bootstrap, engine, trees
    with open(os.path.join(ROOT, "include", "mpfitch.h")) as f:
        src = f.read()
    for name in NAMES:
        assert name + "(" in src and name in engine.EXPORTS
    assert "MPF_ABI_VERSION 8" in src and "typedef struct mpf_bb_summary" in src
    for method in ("split_counts", "split_support", "consensus_tree", "ufboot_summarize", "ufboot_summary_trees"):
        assert callable(getattr(engine.FitchEngine, method))
    assert callable(bootstrap.bb_summary) and callable(trees.lists_to_newick)


def test_the_python_structure_matches_the_header():
    """field order of mpf_bb_summary as the binding lays it out"""
    from mpboot_amd import engine
    with open(os.path.join(ROOT, "include", "mpfitch.h")) as f:
        src = f.read()
    body = src[src.index("typedef struct mpf_bb_summary {"):src.index("} mpf_bb_summary;")]
    pos = [body.index(name) for name, _ in engine.BbSummary._fields_]
    assert pos == sorted(pos)


def test_lists_to_newick_round_trip():
    import numpy as np
    from mpboot_amd import trees
    n = 9
    names = ["t%d" % i for i in range(1, n + 1)]
    back = trees.random_topology(n, np.random.default_rng(4))
    first, nbr = trees.collapse_branches(back, n, ())
    nwk = trees.lists_to_newick(first, nbr, names)
    assert trees.splits(trees.newick_to_back(nwk, names)) == trees.splits(back)
    assert trees.lists_to_newick([0, 3, 6], [1, 2, 6, 5, 3, 4], ["a", "b", "c", "d"], [-1, 7]) == "(a,b,(c,d)7);"
