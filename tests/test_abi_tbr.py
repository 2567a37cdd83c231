"""The TBR entry points are part of the C-ABI: exported, declared, bound, and the ABI number stays 8.  No GPU."""
import ctypes
import os

from helpers import ROOT

NAMES = ("mpf_tbr_scan", "mpf_tbr_sweep_best", "mpf_apply_tbr", "mpf_optimize_tbr", "mpf_get_tbr_moves")


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
    from mpboot_amd import engine, trees
    with open(os.path.join(ROOT, "include", "mpfitch.h")) as f:
        src = f.read()
    assert "MPF_ABI_VERSION 8" in src
    for name in NAMES:
        assert name + "(" in src and name in engine.EXPORTS
    # every comment says that there is no reference function and where row 0 / column 0 coincide with the reference
    assert src.lower().count("no reference function") >= 4
    for cite in ("sprparsimony.cpp:2106-2188", ":2208-2218", ":2259-2376"):
        assert src.count(cite) >= 4, cite
    for method in ("tbr_scan", "tbr_sweep_best", "apply_tbr", "optimize_tbr", "tbr_moves"):
        assert callable(getattr(engine.FitchEngine, method))
    assert callable(trees.apply_tbr)
