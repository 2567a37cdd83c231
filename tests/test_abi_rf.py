"""mpf_rf_distances is part of the C-ABI: exported, declared, bound, its mode constants agree, and the ABI number stays 8.  No GPU."""
import ctypes
import os
import re

from helpers import ROOT


def _lib():
    import __graft_entry__ as g
    path = os.path.join(ROOT, "mpboot_amd", "libmpfitch.so")
    if not os.path.exists(path):
        g.build()
    return ctypes.CDLL(path)


def _header():
    with open(os.path.join(ROOT, "include", "mpfitch.h")) as f:
        return f.read()


def test_the_symbol_is_exported_and_the_abi_is_8():
    lib = _lib()
    assert hasattr(lib, "mpf_rf_distances")
    lib.mpf_abi_version.restype = ctypes.c_int
    assert lib.mpf_abi_version() == 8


def test_header_and_binding_name_it():
    from mpboot_amd import bootstrap, engine
    src = _header()
    assert "mpf_rf_distances(" in src and "mpf_rf_distances" in engine.EXPORTS
    assert "MPF_ABI_VERSION 8" in src
    assert "mtreeset.cpp:484-546" in src and "pda.cpp:1399-1539" in src       # the comment cites the reference lines
    assert callable(engine.FitchEngine.rf_distances) and callable(bootstrap.bb_rf)


def test_the_mode_constants_match_the_header():
    from mpboot_amd import engine
    m = re.search(r"enum \{ MPF_RF_ALL_PAIRS = (\d+), MPF_RF_ADJACENT = (\d+), MPF_RF_TWO_SETS = (\d+) \};", _header())
    assert m is not None
    assert tuple(int(x) for x in m.groups()) == (engine.RF_ALL_PAIRS, engine.RF_ADJACENT, engine.RF_TWO_SETS) == (0, 1, 2)
