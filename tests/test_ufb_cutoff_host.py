"""The cut-off filter every loop that books trees under -bb shares (mpboot_amd/host/ufb_cutoff.hpp) as a stand-alone program
built with -fsanitize=address,undefined, against the reference's rule evaluated in Python:  a tree of length len is saved iff
-len > logl_cutoff - 1e-4  (iqtree.cpp:3343).  No GPU, nothing loaded into python: the program runs as a child process and a
sanitizer report fails the run (a cut-off below -2^32 converts an out-of-range double to a word unless mp_max is clamped)."""
import math
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

SRC = os.path.join(ROOT, "mpboot_amd", "host", "ufb_cutoff_main.cpp")
U32 = 2 ** 32 - 1
LENGTHS = list(range(41)) + [U32]


def _cutoffs():
    out = []
    for L in (1, 7, 1000):
        for c in (-float(L), -float(L) + 1e-4, -float(L) - 1e-4):
            out += [c, math.nextafter(c, math.inf), math.nextafter(c, -math.inf)]
        out.append(-float(L) + 0.5)
    return out + [-1e-4, -5e-5, 1e-4, 3.0, -4294967295.0, -1e12]


CUTOFFS = _cutoffs()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("ufb_cutoff") / "ufb_cutoff")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _passes(length, cutoff):
    return -float(length) > cutoff - 1e-4                # iqtree.cpp:3343


def _run(prog, cutoff, lengths, bases):
    text = "%s\n%d %s\n%d %s\n" % (float(cutoff).hex(), len(lengths), " ".join(map(str, lengths)), len(bases), " ".join(map(str, bases)))
    res = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    lines = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    assert len(lines) == 1 + len(lengths) + len(bases)
    return lines[0], lines[1:1 + len(lengths)], lines[1 + len(lengths):]


@pytest.mark.parametrize("cutoff", CUTOFFS, ids=[c.hex() for c in CUTOFFS])
def test_pass_rule_is_the_references(prog, cutoff):
    (have_cut, none_pass, mp_max), got, _ = _run(prog, cutoff, LENGTHS, [])
    assert have_cut == 1
    assert got == [(n, int(_passes(n, cutoff))) for n in LENGTHS]
    # mp_max is the largest length a word holds that passes; none_pass: not even length 0 does
    assert none_pass == int(not _passes(0, cutoff))
    if not none_pass:
        assert _passes(mp_max, cutoff) and (mp_max == U32 or not _passes(mp_max + 1, cutoff))


def test_without_a_cutoff_everything_passes(prog):
    for zero in (0.0, -0.0):
        head, got, thr = _run(prog, zero, LENGTHS, [0, 1, 40, U32])
        assert head == (0, 0, U32)
        assert got == [(n, 1) for n in LENGTHS]
        assert thr == [(0, U32), (1, U32), (40, U32 - 39), (U32, 1)]


@pytest.mark.parametrize("cutoff", CUTOFFS, ids=[c.hex() for c in CUTOFFS])
def test_part_threshold_is_its_definition(prog, cutoff):
    """cost < threshold  <=>  base + cost <= mp_max:  mp_max - base + 1 from mp_max down, 0 above it (one word: saturated at
    2^32 - 1, which only base 0 under mp_max = 2^32 - 1 reaches)"""
    (_, _, mp_max), _, _ = _run(prog, cutoff, [], [])
    # every base in 0 .. mp_max + 2 where that is a few thousand at most; under the two huge cut-offs the ends of the range
    bases = sorted({b for b in list(range(0, min(mp_max + 2, 4096) + 1)) + [mp_max - 1, mp_max, mp_max + 1, mp_max + 2, U32] if 0 <= b <= U32})
    _, _, thr = _run(prog, cutoff, [], bases)
    assert thr == [(b, min(mp_max - b + 1, U32) if mp_max >= b else 0) for b in bases]


def test_a_cutoff_below_every_word_is_clamped(prog):
    """-1e12: ceil(lim) - 1 does not fit a word -- the conversion is undefined (the sanitizer stops the program) unless clamped"""
    head, got, _ = _run(prog, -1e12, [0, 1, U32 - 1, U32], [])
    assert head == (1, 0, U32)
    assert got == [(0, 1), (1, 1), (U32 - 1, 1), (U32, 1)]
    # ... and the largest cut-off at which the clamp must NOT bite: 2^32 - 2 is the last length that passes
    head, got, _ = _run(prog, -4294967294.0, [U32 - 1, U32], [])
    assert head == (1, 0, U32 - 1)
    assert got == [(U32 - 1, 1), (U32, 0)]
