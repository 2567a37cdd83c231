"""The diagnostic entry of TBR under -bb on the weighted engine is part of the C-ABI: exported, declared, bound, and the ABI number
stays 8; the header names the option that serves the two tracked entries there.  No GPU."""
import ctypes
import os

from helpers import ROOT

NAMES = ("mpf_tbr_pattern_lengths",)


def _lib():
    import __graft_entry__ as g
    path = os.path.join(ROOT, "mpboot_amd", "libmpfitch.so")
    if not os.path.exists(path):
        g.build()
    return ctypes.CDLL(path)


def test_the_symbol_is_exported_and_the_abi_is_8():
    lib = _lib()
    for name in NAMES + ("mpf_ufboot_tbr_sweep", "mpf_ufboot_optimize_tbr", "mpf_tbr_pattern_terms"):
        assert hasattr(lib, name), name
    lib.mpf_abi_version.restype = ctypes.c_int
    assert lib.mpf_abi_version() == 8


def test_header_and_binding_name_it():
    from mpboot_amd import engine
    with open(os.path.join(ROOT, "include", "mpfitch.h")) as f:
        src = f.read()
    assert "MPF_ABI_VERSION 8" in src
    for name in NAMES:
        assert name + "(" in src and name in engine.EXPORTS
    # the header names the option, states what a row is on this engine and keeps the Fitch text
    for word in ("tbr_weighted_tracked", "k_tbr_snk_vals", "row-major order from [0][0]", "its OWN product row", "tbr_book_rows"):
        assert word in src, word
    assert callable(getattr(engine.FitchEngine, "tbr_pattern_lengths"))
