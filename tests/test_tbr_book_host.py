"""The device-free half of a tracked TBR sweep's bookings (mpboot_amd/host/tbr_plan.hpp: book_batches, the batches of a sweep's
entries in booking order; mask_rows, the rows k_tbr_masks writes for a batch and where every entry and every run's home finds its
own) as a stand-alone program, tests/tbr_book_main.cpp, built with -fsanitize=address,undefined, against a plain restatement here.
No GPU, nothing loaded into python: the program runs as a child process and a sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

SRC = os.path.join(ROOT, "tests", "tbr_book_main.cpp")
RUN_COLS = 32                                          # tbrplan::kMaskRunCols


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("tbr_book") / "tbr_book")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _batches(shapes, cap):
    """the sweep's entries in booking order, cut into stretches of at most cap: [[(visit, begin, end)]]"""
    flat = [(v, e) for v, (r, c) in enumerate(shapes) for e in range(r * c)]
    out = []
    for at in range(0, len(flat), cap):
        runs = []
        for v, e in flat[at:at + cap]:
            if runs and runs[-1][0] == v:
                runs[-1][2] = e + 1
            else:
                runs.append([v, e, e + 1])
        out.append([tuple(r) for r in runs])
    return out


def _rows(shapes, runs, take):
    """-> (rows, crow per entry, home per run, {(visit, i, j): row} as the kernel is told to write them)"""
    rows, crow, home, cells = 0, [], [], {}
    for v, b, e in runs:
        home.append(-1)
        for en in range(b, e):
            if en == 0 or not take(v, en):
                crow.append(-1)
                continue
            if home[-1] < 0:
                home[-1] = rows
                cells[(v, 0, 0, "home")] = rows
                rows += 1
            crow.append(rows)
            cells[(v, en // shapes[v][1], en % shapes[v][1], "own")] = rows
            rows += 1
    return rows, crow, home, cells


SWEEPS = {
    "mixed": [(1, 1), (3, 5), (1, 7), (9, 1), (1, 1), (5, 41), (3, 3)],
    "one-large": [(7, 101)],
    "all-1x1": [(1, 1)] * 5,
    "long-row": [(1, 67), (3, 33)],
}


@pytest.mark.parametrize("name", sorted(SWEEPS))
@pytest.mark.parametrize("cap", (1, 2, 7, 64, 10 ** 6))
@pytest.mark.parametrize("mod", (0, 1, 2, 5))
def test_batches_and_mask_rows(prog, tmp_path, name, cap, mod):
    shapes = SWEEPS[name]
    first, total = [], 0
    for r, c in shapes:
        first.append(total)
        total += r * c
    path = str(tmp_path / "in.txt")
    with open(path, "w") as f:
        f.write(f"{len(shapes)} {cap} {mod}\n" + "\n".join(f"{r} {c}" for r, c in shapes) + "\n")
    r = subprocess.run([prog, path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = r.stdout.splitlines()
    want = _batches(shapes, cap)
    assert len(out) == 5 * len(want)
    assert sum(e - b for runs in want for _v, b, e in runs) == total

    def take(v, en):
        return mod == 0 or (first[v] + en) % mod != 0

    for k, runs in enumerate(want):
        lines = out[5 * k:5 * k + 5]
        assert lines[0].split() == ["batch"] + [f"{v}:{b}:{e}" for v, b, e in runs]
        rows, crow, home, cells = _rows(shapes, runs, take)
        assert lines[1] == f"rows {rows}"
        assert [int(x) for x in lines[2].split()[1:]] == crow
        assert [int(x) for x in lines[3].split()[1:]] == home
        # every row is written once, by the cell it belongs to; a run is one matrix row of one visit with at most RUN_COLS columns
        got = {}
        for tok in lines[4].split()[1:]:
            v, i, cols = tok.split(":")
            cols = [tuple(int(x) for x in c.split(">")) for c in cols.split(",")]
            assert 1 <= len(cols) <= RUN_COLS
            for j, o in cols:
                assert o not in got and 0 <= o < rows
                got[o] = (int(v), int(i), j)
        assert len(got) == rows
        assert sorted(got.items()) == sorted((o, (v, i, j)) for (v, i, j, _kind), o in cells.items())
        # an entry that takes part finds a home row in front of it in its own run
        at = 0
        for ri, (v, b, e) in enumerate(runs):
            for en in range(b, e):
                if crow[at] >= 0:
                    assert 0 <= home[ri] < crow[at]
                at += 1
