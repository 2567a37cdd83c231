"""The tiles of a TBR visit on the weighted (-cost) engine (mpboot_amd/host/tbr_plan.hpp: tile_dims, pick and tiles with the engine
kind) as a stand-alone program, tests/tbr_plan_snk_main.cpp, built with -fsanitize=address,undefined.  No GPU, nothing loaded into
python: the program runs as a child process and a sanitizer report fails the run.

The weighted rows of the one shape table (host/pair_tile.hpp): narrow 4 x 16 for every alphabet; wide 64 x 64 for 4 AND for 20 state
rows (the Fitch engine gives 20 rows 32 x 32), 32 x 32 for 32.  The pick on the weighted engine (measured): narrow while
the visit's matrix has fewer than 2^18 entries, wide from there on; the defaulted parameter still gives the Fitch engine's table and
rule."""
import os
import shutil
import subprocess

import pytest

import tbr_witness as tw
from helpers import ROOT

SRC = os.path.join(ROOT, "tests", "tbr_plan_snk_main.cpp")
WIDE = {4: 64, 20: 64, 32: 32}


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("tbr_plan_snk") / "tbr_plan_snk")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _pick(rows, cols, tile):
    if tile:
        return tile
    return 1 if rows * cols < 2 ** 18 else 2


@pytest.mark.parametrize("S", (4, 20, 32))
def test_tile_lists_and_pick_under_the_weighted_table(prog, tmp_path, S):
    t = WIDE[S]
    sides = sorted({1, 3, 5, 15, 17, t - 1, t + 1, 2 * t - 1, 2 * t + 1, 3 * t + 1, 255, 511, 513})      # (matrix sides are odd; 511 x 513 = 2^18 - 1)
    cases = [(S, r, c, tile) for r in sides for c in sides for tile in (0, 1, 2)]
    path = str(tmp_path / "in.txt")
    with open(path, "w") as f:
        f.write("".join(f"{s} {r} {c} {tile}\n" for s, r, c, tile in cases))
    r = subprocess.run([prog, path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == 4 * len(cases)
    picked, differ = set(), 0
    for k, (_s, rows, cols, tile) in enumerate(cases):
        dims, plain, pick, items = (line.split() for line in out[4 * k:4 * k + 4])
        assert dims == ["dims", "4", "16", str(t), str(t)]
        # the defaulted parameter is the Fitch engine's table and rule, as tests/tbr_witness.py restates them
        tp = 64 if S == 4 else 32
        assert plain == ["plain", str(tp), str(tp), str(tw.tile_shape(S, rows, cols, tile))]
        shape = _pick(rows, cols, tile)
        assert pick == ["pick", str(shape)]
        tf, tg = (4, 16) if shape == 1 else (t, t)
        want = [] if rows * cols == 1 else [f"{i}:{j}" for i in range(-(-rows // tf)) for j in range(-(-cols // tg))]
        assert items[0] == "items" and items[1:] == want, (rows, cols, tile)
        if tile == 0:
            picked.add(shape)
            differ += plain[3] != pick[1]
    assert picked == {1, 2}                                   # the rule took both shapes among the cases: 511 x 513 narrow, 513 x 513 wide
    assert differ > 0                                         # ... and is not the Fitch engine's (17 x 17: wide there, narrow here)
