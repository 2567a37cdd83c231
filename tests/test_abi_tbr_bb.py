"""The entry points of TBR under -bb are part of the C-ABI: exported, declared, bound, and the ABI number stays 8.  No GPU."""
import ctypes
import os

from helpers import ROOT

NAMES = ("mpf_ufboot_tbr_sweep", "mpf_ufboot_optimize_tbr", "mpf_tbr_pattern_terms")


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
    from mpboot_amd import engine
    with open(os.path.join(ROOT, "include", "mpfitch.h")) as f:
        src = f.read()
    assert "MPF_ABI_VERSION 8" in src
    for name in NAMES:
        assert name + "(" in src and name in engine.EXPORTS
    # the header states the semantics (there is no reference function) and names the options
    for word in ("row-major order from [0][0]", "tbr_book_rows", "tbr_booked", "tbr_book_batches"):
        assert word in src, word
    for method in ("ufboot_tbr_sweep", "ufboot_optimize_tbr", "tbr_pattern_terms"):
        assert callable(getattr(engine.FitchEngine, method))
