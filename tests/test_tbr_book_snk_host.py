"""The device-free half of a tracked TBR sweep's bookings on the weighted engine (mpboot_amd/host/tbr_plan.hpp: value_bits, the
host-side bound on the bit planes; book_cap, the automatic batch cap; and the batches and row lists that cap leads to) as a
stand-alone program, tests/tbr_book_snk_main.cpp, built with -fsanitize=address,undefined, against a plain restatement here.
No GPU, nothing loaded into python: the program runs as a child process and a sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT
from test_tbr_book_host import SWEEPS, _batches, _rows

SRC = os.path.join(ROOT, "tests", "tbr_book_snk_main.cpp")
MIB = 1 << 20


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("tbr_book_snk") / "tbr_book_snk")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _bits(top):
    return max(1, min(16, int(top).bit_length()))


def _cap(npat, plane_words, samples_p, bits, tile, limit):
    """half the largest whole number of row tiles whose 16-bit rows, `bits` bit planes and product each stay within limit"""
    rows = 0
    while all((rows + tile) * per <= limit for per in (2 * npat, 4 * bits * plane_words, 4 * samples_p)):
        rows += tile
    return max(1, rows // 2)


# (npat, plane words, padded samples, top = taxa x highest cost, row tile, limit): the three terms each deciding once, a bound of
# 16 bits and more, one bit, and limits that leave room for one tile, for none and for an odd number of tiles
GEOMETRIES = {
    "c2-tstv": (10016, 320, 1024, 200 * 3, 512, 256 * MIB),
    "c5-metric": (20000, 632, 1024, 500 * 40, 512, 256 * MIB),
    "many-samples": (64, 8, 100000, 70000, 512, 256 * MIB),
    "planes-decide": (32, 4096, 128, 65535, 512, 64 * MIB),
    "one-bit": (96, 8, 128, 1, 4, 4096),
    "one-tile": (96, 8, 128, 9, 4, 4 * 4 * 128),
    "no-tile": (96, 8, 128, 9, 4, 100),
    "three-tiles": (96, 8, 128, 255, 2, 3 * 2 * 4 * 128 + 17),
}


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("name", sorted(SWEEPS))
@pytest.mark.parametrize("mod", (0, 1, 3))
def test_cap_batches_and_rows(prog, tmp_path, geo, name, mod):
    npat, pw, sp, top, tile, limit = GEOMETRIES[geo]
    shapes = SWEEPS[name]
    first, total = [], 0
    for r, c in shapes:
        first.append(total)
        total += r * c
    path = str(tmp_path / "in.txt")
    with open(path, "w") as f:
        f.write(f"{len(shapes)} {mod} {npat} {pw} {sp} {top} {tile} {limit}\n" + "\n".join(f"{r} {c}" for r, c in shapes) + "\n")
    r = subprocess.run([prog, path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = r.stdout.splitlines()
    bits = _bits(top)
    cap = _cap(npat, pw, sp, bits, tile, limit)
    assert out[0] == f"bits {bits}" and out[1] == f"cap {cap}"
    # the bound holds: a value of at most `top` has at most `bits` bits (16 is the row's width)
    assert top < (1 << bits) or bits == 16

    def take(v, en):
        return mod == 0 or (first[v] + en) % mod != 0

    want = _batches(shapes, cap)
    assert len(out) == 2 + 3 * len(want)
    for k, runs in enumerate(want):
        lines = out[2 + 3 * k:5 + 3 * k]
        assert lines[0].split() == ["batch"] + [f"{v}:{b}:{e}" for v, b, e in runs]
        rows, _crow, _home, cells = _rows(shapes, runs, take)
        assert lines[1] == f"rows {rows}"
        # what the cap promises: at most two rows an entry, so the padded rows of a batch stay within the limit in all three buffers
        # (unless not even one tile does)
        assert rows <= 2 * cap
        padded = -(-rows // tile) * tile
        for per in (2 * npat, 4 * bits * pw, 4 * sp):
            assert padded * per <= max(limit, tile * per)
        got = {}
        for tok in lines[2].split()[1:]:
            v, i, cols = tok.split(":")
            for c in cols.split(","):
                j, o = (int(x) for x in c.split(">"))
                assert o not in got and 0 <= o < rows
                got[o] = (int(v), int(i), j)
        assert sorted(got.items()) == sorted((o, (v, i, j)) for (v, i, j, _kind), o in cells.items())


def test_the_geometries_cover_every_term(prog):
    """each of the three buffers decides the cap in one geometry at least, and the automatic cap of the two timed workloads is far
    above a visit's matrix at radius 3"""
    decides = set()
    for npat, pw, sp, top, _tile, _limit in GEOMETRIES.values():
        per = (2 * npat, 4 * _bits(top) * pw, 4 * sp)
        decides.add(per.index(max(per)))
    assert decides == {0, 1, 2}
    for geo in ("c2-tstv", "c5-metric"):
        npat, pw, sp, top, tile, limit = GEOMETRIES[geo]
        assert _cap(npat, pw, sp, _bits(top), tile, limit) >= 1024
