"""What a TBR visit is as far as it follows from back[] alone (mpboot_amd/host/tbr_plan.hpp: the two lists with their depths, the
chain program of a side, the chunks of a sweep, the tile list of a chunk, the edit, the first-minimum rule) as a stand-alone
program, tests/tbr_plan_main.cpp, built with -fsanitize=address,undefined, against tests/tbr_witness.py.  No GPU, nothing loaded into
python: the program runs as a child process and a sanitizer report fails the run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import splits_witness as sw
import tbr_witness as tw
from helpers import ROOT
from mpboot_amd import trees

SRC = os.path.join(ROOT, "tests", "tbr_plan_main.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("tbr_plan") / "tbr_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _run(prog, path, n, maxtrav, cap, tile, S, back, recs, edits):
    with open(path, "w") as f:
        f.write(f"{n} {maxtrav} {cap} {tile} {S} {len(recs)} {len(edits)}\n")
        f.write(" ".join(str(int(x)) for x in back) + "\n" + " ".join(str(int(x)) for x in recs) + "\n")
        f.write(" ".join(f"{p} {f_} {g}" for p, f_, g in edits) + "\n")
    r = subprocess.run([prog, path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def _slot(n, r):
    v = r // 3
    return v - 1 if v <= n else n + 3 * (v - n - 1) + r % 3


def _replay(wit, views, n, ops):
    """the chain program run on the witness's views: root sets in the order of their `out` numbers"""
    by_slot = {_slot(n, r): v[0] for r, v in views.items()}
    level, out = {}, {}
    for tok in ops:
        kind, d, own, sib, o = (int(x) for x in tok.split(":"))
        if kind == 1:
            level[0] = by_slot[own]
            continue
        level[d] = wit._join(level[d - 1], by_slot[sib])[0]
        out[o] = wit._join(level[d], by_slot[own])[0]
    return [out[k] for k in sorted(out)], sorted(out)


def _trees(n):
    rng = np.random.default_rng(n)
    return [trees.random_topology(n, rng), sw.caterpillar(n)]


@pytest.mark.parametrize("n", (4, 5, 8, 13, 40))
def test_lists_programs_chunks_tiles_and_edits(prog, tmp_path, n):
    codes, w = tw.alignment(n, 40, "dna", n)
    wit = tw.TbrWitness(codes, w, 0)
    rng = np.random.default_rng(50 + n)
    for back in _trees(n):
        views = wit.views(back)
        recs = tw.node_order(back, n) + [3 * v + s for v in range(n + 1, 2 * n - 1) for s in (1, 2)]
        for maxtrav, cap, tile, S in ((1, 1, 0, 4), (3, 7, 0, 20), (255, 40, 1, 4), (6, 10 ** 9, 2, 32)):
            want = [tw.lists(back, n, p, maxtrav) for p in recs]
            edits = []
            for p, (F, G) in zip(recs, want):
                fr, gr = [tw.NONE] + [r for r, _ in F], [tw.NONE] + [r for r, _ in G]
                edits.append((p, fr[int(rng.integers(len(fr)))], gr[int(rng.integers(len(gr)))]))
            out = _run(prog, str(tmp_path / "in.txt"), n, maxtrav, cap, tile, S, back, recs, edits)
            at = 0
            for p, (F, G) in zip(recs, want):
                assert out[at] == f"visit {p} {int(back[p])}"
                assert out[at + 1].split()[1:] == [f"{r}:{d}" for r, d in F] and out[at + 2].split()[1:] == [f"{r}:{d}" for r, d in G]
                for s, x in ((0, int(back[p])), (1, p)):
                    toks = out[at + 3 + s].split()
                    assert toks[:2] == ["ops", str(s)]
                    sets, numbers = _replay(wit, views, n, toks[2:])
                    mine = wit.root_sets(back, views, x, maxtrav)
                    assert numbers == list(range(100 * s, 100 * s + len(mine))) and all((a == b).all() for a, b in zip(sets, mine))
                at += 5
            need = [len(F) + len(G) for F, G in want]
            cells = [(1 + len(F)) * (1 + len(G)) for F, G in want]
            chunks = tw.chunks(need, cap, cells)
            assert out[at] == " ".join(["chunks"] + [f"{b}:{e}" for b, e in chunks])
            at += 1
            t = 64 if S == 4 else 32
            for b, e in chunks:
                items = {1: [], 2: []}
                for k in range(b, e):
                    rows, cols = 1 + len(want[k][0]), 1 + len(want[k][1])
                    if rows * cols == 1:
                        continue
                    shape = tw.tile_shape(S, rows, cols, tile)
                    tf, tg = (4, 16) if shape == 1 else (t, t)
                    items[shape] += [f"{shape}:{k - b}:{i}:{j}" for i in range(-(-rows // tf)) for j in range(-(-cols // tg))]
                assert out[at].split()[1:] == items[1] + items[2]
                at += 1
            rows = np.array([[1 + len(F) for F, _ in want]])
            best = tw.first_min(rows)
            assert out[at] == ("best 4294967295 -1" if best is None else f"best {best[0]} {best[2]}")
            at += 1
            for (p, f, g), line in zip(edits, out[at:]):
                new = trees.apply_tbr(back, p, f, g)
                trees.validate(new, n)
                assert [int(x) for x in line.split()[1:]] == new.tolist()
            assert len(out) == at + len(edits)
