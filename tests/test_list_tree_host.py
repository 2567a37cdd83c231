"""What follows from a tree's neighbour lists alone (mpboot_amd/host/list_tree.hpp: the one hand-over check, the walk and branch
order, the plan of the view launch, the two sides of every branch) as a stand-alone program built with
-fsanitize=address,undefined, against the Python witnesses of the three features that read such trees (polytomy_witness,
split_lists_witness, place_witness).  No GPU, nothing loaded into python: the program runs as a child process and a sanitizer
report fails the run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import place_witness as plw
import polytomy_witness as pw
import split_lists_witness as lw
import splits_witness as sw
from helpers import ROOT
from mpboot_amd import trees
from test_place_host import _rows, _run, _write

SRC = os.path.join(ROOT, "mpboot_amd", "host", "list_tree_main.cpp")
SIZES = (4, 5, 12, 33, 65)
P = 70


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("list_tree") / "list_tree")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _ints(line):
    return [int(x) for x in line.split()[1:]]


def _polytomies(n):
    """the star, a fully resolved tree, a hub in the middle, a caterpillar contracted to one deep chain, a random contraction"""
    rng = np.random.default_rng(300 + n)
    backs = sw.related_trees(n, 2, 11 + n, 3)
    items = [lw.star(n), trees.back_to_lists(backs[0], n)]
    if n >= 5:
        cat = sw.caterpillar(n)
        items += [lw.middle_hub(n), trees.collapse_branches(cat, n, lw.inner_branches(cat, n)[::2]), lw.collapse(backs[1], n, (n - 3 + 1) // 2, rng)]
    return items


def _backbones(n, rng):
    """binary backbones over 3, n / 2 and n - 1 of the tips -> (first, nbr, present, absent)"""
    out = []
    for m in sorted({3, max(3, n // 2), n - 1}):
        present = rng.permutation(n)[:m] + 1
        first, nbr = plw.backbone(n, present, rng)
        out.append((first, nbr, present.tolist(), [t for t in range(1, n + 1) if t not in present.tolist()]))
    return out


def _alignment(n, seed):
    rng = np.random.default_rng(seed)
    codes = (1 << rng.integers(0, 4, size=(n, P))).astype(np.uint8)
    return np.where(rng.random((n, P)) < 0.1, rng.integers(1, 16, size=(n, P)), codes).astype(np.uint8)


def _check_walk(out, first, nbr, n, root):
    br = plw.walk(first, nbr, n, root)
    assert out[0] == "ok"
    assert _ints(out[1]) == [root] + [v for _, v in br]
    parent = _ints(out[2])
    assert len(parent) == n + len(first) - 1 and parent[root - 1] == 0
    for dad, v in br:
        assert parent[v - 1] == dad
    occur = {root} | {v for _, v in br}
    assert all(parent[v - 1] == -1 for v in range(1, n + 1) if v not in occur)
    assert _ints(out[3]) == [v for ab in br for v in ab]
    return br


@pytest.mark.parametrize("n", SIZES)
def test_check_and_walk(prog, tmp_path, n):
    p = str(tmp_path / "t.bin")
    rng = np.random.default_rng(n)
    for first, nbr, present, _absent in _backbones(n, rng):
        for root in (present[0], present[-1]):
            _check_walk(_run(prog, "check", _write(p, n, first, nbr, root), "absent"), first, nbr, n, root)
            assert _run(prog, "place", p) == ["ok"]
            # absent tips are legal for insertion alone
            assert (_run(prog, "check", p)[0] == "ok") == (len(present) == n)
    for first, nbr in _polytomies(n):
        for root in (1, n):
            br = _check_walk(_run(prog, "check", _write(p, n, first, nbr, root)), first, nbr, n, root)
            assert br == pw.rooted(first, nbr, n, root)[0] and len(br) == n + len(first) - 2
            if root == 1:
                assert br == lw.branch_walk(first, nbr, n)
            binary = all(int(first[i + 1] - first[i]) == 3 for i in range(len(first) - 1))
            assert _run(prog, "place", p)[0].split(":")[0] == ("ok" if binary else "unsupported")


def test_the_three_catalogues_of_malformed_lists(prog, tmp_path):
    p = str(tmp_path / "t.bin")
    # the polytomy calls: every tip must occur
    assert _run(prog, "check", _write(p, 5, *pw.GOOD5, 1))[0] == "ok" and pw.validate(*pw.GOOD5, 5) is None
    for name, n, first, nbr in pw.MALFORMED:
        assert pw.validate(first, nbr, n) is not None, name
        assert _run(prog, "check", _write(p, n, first, nbr, 1))[0].startswith("invalid: "), name
        # none of them is a tree over a subset of the tips either ("tip missing" lists tip 4 twice)
        assert plw.check(first, nbr, n, 1) == "invalid" and _run(prog, "place", p)[0].startswith("invalid: "), name
        assert _run(prog, "check", p, "absent")[0].startswith("invalid: "), name
    # the trees of a set: root leaf 1, every tip must occur
    assert _run(prog, "check", _write(p, 9, *lw.broken_lists("good"), 1))[0] == "ok"
    for kind in lw.BROKEN:
        first, nbr = lw.broken_lists(kind)
        assert _run(prog, "check", _write(p, 9, first, nbr, 1))[0].startswith("invalid: "), kind
        # a missing tip is no defect of a backbone; that backbone has a node of degree 5
        assert _run(prog, "check", p, "absent")[0].startswith("invalid: ") == (kind != "missing_tip"), kind
        want = "unsupported" if kind == "missing_tip" else "invalid"
        assert _run(prog, "place", p)[0].split(":")[0] == want == plw.check(first, nbr, 9, 1), kind
    # taxon insertion, through its wrapper
    assert _run(prog, "place", _write(p, 9, *plw.GOOD, 1)) == ["ok"]
    assert _run(prog, "check", p, "absent")[0] == "ok" and _run(prog, "check", p)[0].startswith("invalid: ")
    for name, (first, nbr, root, verdict) in plw.MALFORMED.items():
        out = _run(prog, "place", _write(p, 9, first, nbr, root))
        assert out[0].startswith(verdict + ": ") and plw.check(first, nbr, 9, root) == verdict, name
        # the polytomy calls refuse all of them: tips 6 .. 9 are absent throughout
        assert _run(prog, "check", p)[0].startswith("invalid: "), name
        # the tree of degree 4 is a tree: what refuses it is a rule of insertion alone ("two tips" pads its list with the node itself)
        assert (_run(prog, "check", p, "absent")[0] == "ok") == (name == "degree 4"), name


def _plan(out, n, first, all_views, fitch):
    """the printed plan, with the conditions every plan meets"""
    n_inner, E = len(first) - 1, int(first[-1])
    lev = _ints(next(x for x in out if x.startswith("levels")))
    items = [_ints(x) for x in out if x.startswith("item ")]
    outs = [_ints(x) for x in out if x.startswith("out ")]
    inputs = _ints(next(x for x in out if x.startswith("inputs")))
    n_rows = _ints(out[0])[0]
    # levels partition the items; the items partition the inputs and the outputs
    assert lev[0] == 0 and lev[-1] == len(items) and all(a <= b for a, b in zip(lev, lev[1:]))
    for begin, count, total in ((0, 1, len(inputs)), (2, 3, len(outs))):
        spans = sorted((i[begin], i[begin] + i[count]) for i in items)
        assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    # every input is a tip slot or the dst of an output of a strictly lower level; no dst is written twice
    level_of_dst, ups = {}, 0
    for l in range(len(lev) - 1):
        made = []
        for it in items[lev[l]:lev[l + 1]]:
            for s in inputs[it[0]:it[0] + it[1]]:
                assert 0 <= s < n or level_of_dst.get(s, l) < l, (s, l)
            for dst, excl, _row in outs[it[2]:it[2] + it[3]]:
                assert excl == -1 or excl in inputs[it[0]:it[0] + it[1]]
                if dst >= 0:
                    made.append(dst)
            ups += it[3] == 1 and outs[it[2]][0] >= 0 and outs[it[2]][1] == -1
        for dst in made:
            assert dst not in level_of_dst and n <= dst < n + E
            level_of_dst[dst] = l
    assert ups == n_inner and len(items) == n_inner * (2 if all_views else 1) + (1 if fitch else 0)
    assert len(level_of_dst) == (E if all_views else n_inner)            # every directed view of the inner nodes | the up views
    rows = sorted(o[2] for o in outs if o[2] >= 0)
    # Fitch: one step-mask row per up item and one for the root edge; the weighted engine keeps no step masks
    assert n_rows == (ups + 1 if fitch else 0) and rows == list(range(n_rows))
    return n_rows


@pytest.mark.parametrize("n", SIZES)
def test_plan_carried_out_on_the_host(prog, tmp_path, n):
    p = str(tmp_path / "t.bin")
    codes = _alignment(n, n)
    tips = _rows(plw.tip_sets(codes, 0), 4)
    poly = pw.PolyWitness(codes, np.ones(P, dtype=np.int64), 0)
    place = plw.PlaceWitness(codes, np.ones(P, dtype=np.int64), 0)
    for first, nbr in _polytomies(n):
        for root in (1, n):
            _write(p, n, first, nbr, root, (), tips)
            length = poly.parsimony(first, nbr, root)[0]
            out = _run(prog, "plan", p, "up", "fitch")
            _plan(out, n, first, False, True)
            assert out[-1] == "length %d" % length
            out = _run(prog, "plan", p, "all", "fitch")
            _plan(out, n, first, True, True)
            br, subst = poly.substitutions(first, nbr, root)
            assert next(x for x in out if x.startswith("length")) == "length %d" % length
            assert _ints(next(x for x in out if x.startswith("subst"))) == subst.tolist() and len(br) == len(subst)
            for views in ("up", "all"):
                _plan(_run(prog, "plan", p, views, "weighted"), n, first, views == "all", False)
    rng = np.random.default_rng(n)
    for first, nbr, present, absent in _backbones(n, rng):
        for root in (present[0], present[-1]):
            _write(p, n, first, nbr, root, absent, tips)
            _br, cost, length = place.view_costs(first, nbr, absent, root)
            out = _run(prog, "plan", p, "all", "fitch", "absent")
            _plan(out, n, first, True, True)
            assert next(x for x in out if x.startswith("length")) == "length %d" % length
            assert _ints(next(x for x in out if x.startswith("subst"))) == poly.substitutions(first, nbr, root)[1].tolist()
            assert [_ints(x)[1:] for x in out if x.startswith("row ")] == cost.tolist()
            out = _run(prog, "plan", p, "up", "fitch", "absent")
            _plan(out, n, first, False, True)
            assert out[-1] == "length %d" % length
