"""The taxon-insertion entry points are part of the C-ABI: exported, declared, bound, and the ABI number stays 8.  No GPU."""
import ctypes
import os

from helpers import ROOT

NAMES = ("mpf_insertion_costs", "mpf_place_taxa", "mpf_iq_parsimony_tree")


def _lib():
    import __graft_entry__ as g
    path = os.path.join(ROOT, "mpboot_amd", "libmpfitch.so")
    if not os.path.exists(path):
        g.build()
    return ctypes.CDLL(path)


def test_the_three_symbols_are_exported_and_the_abi_is_8():
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.mpf_abi_version.restype = ctypes.c_int
    assert lib.mpf_abi_version() == 8


def test_header_and_binding_name_them():
    from mpboot_amd import engine, trees
    with open(os.path.join(ROOT, "include", "mpfitch.h")) as f:
        src = f.read()
    for name in NAMES:
        assert name + "(" in src and name in engine.EXPORTS
    for method in ("insertion_costs", "place_taxa", "iq_parsimony_tree"):
        assert callable(getattr(engine.FitchEngine, method))
    assert callable(trees.insert_tip) and callable(trees.drop_tips)
