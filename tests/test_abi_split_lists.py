"""The four split products on mixed tree sets are part of the C-ABI: exported, declared, bound, and the ABI number stays 8.  No GPU."""
import ctypes
import os

from helpers import ROOT

NAMES = ("mpf_split_counts_set", "mpf_split_support_set", "mpf_consensus_tree_set", "mpf_rf_distances_set")


def _lib():
    import __graft_entry__ as g
    path = os.path.join(ROOT, "mpboot_amd", "libmpfitch.so")
    if not os.path.exists(path):
        g.build()
    return ctypes.CDLL(path)


def _header():
    with open(os.path.join(ROOT, "include", "mpfitch.h")) as f:
        return f.read()


def test_the_symbols_are_exported_and_the_abi_is_8():
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.mpf_abi_version.restype = ctypes.c_int
    assert lib.mpf_abi_version() == 8


def test_header_and_binding_name_them():
    import inspect

    from mpboot_amd import bootstrap, engine, trees
    src = _header()
    for name in NAMES:
        assert name + "(" in src and name in engine.EXPORTS
    assert "MPF_ABI_VERSION 8" in src and "typedef struct mpf_tree_set" in src
    # the struct of the binding has the header's fields, in order
    assert [f for f, _ in engine.TreeSet._fields_] == ["n_records", "backs", "n_lists", "n_inner", "first", "nbr"]
    # the sentence that such trees are not taken is gone
    assert "are not\n   taken" not in src and "record-format trees only" not in src
    for meth, kw in ((engine.FitchEngine.split_counts, "lists"), (engine.FitchEngine.split_support, "target_lists"),
                     (engine.FitchEngine.consensus_tree, "lists"), (engine.FitchEngine.rf_distances, "lists2")):
        assert inspect.signature(meth).parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
    assert "consensus" in inspect.signature(bootstrap.bb_rf).parameters and callable(trees.back_to_lists)
