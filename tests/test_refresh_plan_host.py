"""The host-only planner of the view refresh (mpboot_amd/host/refresh_plan.hpp: the closure of stale inputs with its dependency
levels, the from-scratch two-sweep shortcut, the level layout, the cut into chains and the topology deltas) as a stand-alone
program built with -fsanitize=address,undefined (mpboot_amd/host/refresh_plan_main.cpp).  No GPU, nothing loaded into python: the
program runs as a child process, executes every plan on 64-bit stand-ins for the vectors and reports a plan that reads a stale
vector, writes one twice, leaves a requested root stale or lays the levels out wrongly; any output on stderr fails the test.

This file makes the cases: trees, validity flags as the engine's rules leave them (Engine::invalidate_node around an edit, the
closure of the roots behind a refresh) and root lists as Engine::collect_scan_roots makes them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import splits_witness as sw
from helpers import ROOT
from mpboot_amd import trees

SRC = os.path.join(ROOT, "mpboot_amd", "host", "refresh_plan_main.cpp")
nx = trees.nxt


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("refresh_plan") / "refresh_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


def _records(n):
    return 3 * (2 * n - 1) + 3


def _full_back(back, n):
    b = np.full(_records(n), -1, dtype=np.int32)
    b[:len(back)] = back
    return b


def _invalidate_node(back, valid, n, node):
    """Engine::invalidate_node: the node's own three vectors and, walking outwards, the two outward-looking vectors of every node
    reached, until vectors that are invalid already"""
    if node <= n:
        return
    stack = []
    for s in range(3):
        r = 3 * node + s
        valid[r] = 0
        w = int(back[r])
        if w >= 0 and w // 3 > n:
            stack.append(w)
    while stack:
        w = stack.pop()
        for r in (nx(w), nx(nx(w))):
            if not valid[r]:
                continue
            valid[r] = 0
            u = int(back[r])
            if u >= 0 and u // 3 > n:
                stack.append(u)


def _refresh(back, valid, n, roots):
    """what a refresh of `roots` leaves valid: the roots and every stale input behind them; returns how many vectors that were"""
    count = 0
    stack = [int(r) for r in roots]
    while stack:
        r = stack.pop()
        if r < 0 or r // 3 <= n or valid[r]:
            continue
        valid[r] = 1
        count += 1
        stack += [int(back[nx(r)]), int(back[nx(nx(r))])]
    return count


def _scan_roots(back, n, p, maxtrav):
    """Engine::collect_scan_roots: both ends of the prune branch, the two gap ends of each inner end and every record the walk of
    the insertion branches visits within maxtrav"""
    maxtrav = min(maxtrav, n - 3)
    roots = []
    if maxtrav < 1:
        return roots
    roots += [p, int(back[p])]
    for x in (p, int(back[p])):
        if x // 3 <= n:
            continue
        x1, x2 = int(back[nx(x)]), int(back[nx(nx(x))])
        roots += [int(back[x]), x1, x2]
        for a in (x1, x2):
            if a // 3 <= n:
                continue
            st = [(int(back[nx(nx(a))]), 1), (int(back[nx(a)]), 1)]
            while st:
                q, d = st.pop()
                roots.append(q)
                if q // 3 > n and d < maxtrav:
                    st += [(int(back[nx(nx(q))]), d + 1), (int(back[nx(q)]), d + 1)]
    return roots


def _random_edit(back, n, rng):
    """one SPR (an NNI when the regraft branch is next to the prune branch) that leaves a tree"""
    while True:
        p = 3 * int(rng.integers(n + 1, 2 * n - 1)) + int(rng.integers(0, 3))
        cand, stack = [], [int(back[nx(p)]), int(back[nx(nx(p))])]
        while stack:
            x = stack.pop()
            cand.append(x)
            if x // 3 > n:
                stack += [int(back[nx(x)]), int(back[nx(nx(x))])]
        q = cand[int(rng.integers(0, len(cand)))]
        b = trees.apply_spr(back, p, q)
        trees.validate(b[:3 * (2 * n - 1)], n)
        if (b != back).any() or n == 4:
            return b


def _edited(back, valid, n, rng, k):
    """k edits of a tree: the links, the validity flags and the records whose entry of the topology array changed"""
    old = back
    for _ in range(k):
        b = _random_edit(back, n, rng)
        for v in sorted({int(r) // 3 for r in np.nonzero(b != back)[0]}):
            _invalidate_node(back, valid, n, v)
            _invalidate_node(b, valid, n, v)
        back = b
    nodes = sorted({int(r) // 3 for r in np.nonzero(back != old)[0] if int(r) // 3 > n})
    return back, [3 * v + s for v in nodes for s in range(3)]


class Cases:
    def __init__(self):
        self.blob, self.want = [], []

    def add(self, n, back, valid, roots, klist, old, ops, min_chains=0):
        """roots None: the whole tree; klist None: the topology array is rebuilt wholesale"""
        head = [n, 3, -1 if roots is None else len(roots), -1 if klist is None else len(klist)]
        parts = [head, back, valid, roots or [], klist or []] + ([old] if klist is not None else [])
        self.blob += [np.asarray(p, dtype=np.int32) for p in parts]
        self.want.append((ops, min_chains))

    def run(self, prog, path):
        with open(path, "wb") as f:
            for a in self.blob:
                a.tofile(f)
        r = subprocess.run([prog, path], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(self.want)
        for i, (line, (ops, min_chains)) in enumerate(zip(lines, self.want)):
            tok = line.split()
            assert tok[:2] == ["case", str(i)]
            got = dict(zip(tok[2::2], (int(x) for x in tok[3::2])))
            assert got["ops"] == ops, line
            assert (got["levels"] > 0) == (ops > 0) and got["max_chains"] >= min_chains, line
        return lines


SHAPES = [("random", 4), ("random", 5), ("caterpillar", 33), ("balanced", 33), ("random", 37), ("random", 300)]


def _shape(kind, n, rng):
    b = {"random": lambda: trees.random_topology(n, rng), "caterpillar": lambda: sw.caterpillar(n), "balanced": lambda: sw.balanced(n)}[kind]()
    return _full_back(b, n)


@pytest.mark.parametrize("kind,n", SHAPES, ids=["%s%d" % s for s in SHAPES])
def test_plans_execute(prog, tmp_path, kind, n):
    rng = np.random.default_rng(1000 + n)
    back = _shape(kind, n, rng)
    R = _records(n)
    nops = 3 * (n - 2)
    cs = Cases()
    # nothing valid, the whole tree (n = 4: one inner branch, 6 ops)
    cs.add(n, back, np.zeros(R), None, None, None, nops)
    # everything valid: no op at all
    valid = np.zeros(R, dtype=np.int32)
    assert _refresh(back, valid, n, range(3 * (n + 1), 3 * (2 * n - 1))) == nops
    cs.add(n, back, valid, None, [], back, 0)
    for k in (1, 2, 3):
        # k edits of a fully valid tree, then the whole tree
        v = valid.copy()
        b, klist = _edited(back, v, n, rng, k)
        stale = int((v[3 * (n + 1):3 * (2 * n - 1)] == 0).sum())
        cs.add(n, b, v, None, klist, back, stale)
        # ... or only what the scans of one prune node read, then another one's, then the rest
        p = 3 * int(rng.integers(n + 1, 2 * n - 1)) + int(rng.integers(0, 3))
        roots = _scan_roots(b, n, p, int(rng.integers(1, 7)))
        v1 = v.copy()
        cs.add(n, b, v, roots, klist, back, _refresh(b, v1, n, roots))
        p2 = 3 * int(rng.integers(n + 1, 2 * n - 1)) + int(rng.integers(0, 3))
        roots2 = _scan_roots(b, n, p2, 6)
        v2 = v1.copy()
        cs.add(n, b, v1, roots2, [], b, _refresh(b, v2, n, roots2))
        cs.add(n, b, v2, None, [], b, int((v2[3 * (n + 1):3 * (2 * n - 1)] == 0).sum()))
    # nothing valid and root lists that cover part of the tree; the topology array wholesale, as after a new tree
    v = np.zeros(R, dtype=np.int32)
    for maxtrav in (1, 3, 6):
        p = 3 * int(rng.integers(n + 1, 2 * n - 1)) + int(rng.integers(0, 3))
        roots = _scan_roots(back, n, p, maxtrav)
        before = v.copy()
        cs.add(n, back, before, roots, None, None, _refresh(back, v, n, roots))
    cs.run(prog, str(tmp_path / "cases.bin"))


def test_a_level_of_more_than_sixteen_chains(prog, tmp_path):
    """160 taxa, nothing valid: the chains of the first level outnumber the 16 waves of a workgroup and are sorted by length"""
    n = 160
    back = _full_back(trees.random_topology(n, np.random.default_rng(7)), n)
    cs = Cases()
    cs.add(n, back, np.zeros(_records(n)), None, None, None, 3 * (n - 2), min_chains=17)
    cs.run(prog, str(tmp_path / "chains.bin"))


def test_a_wrong_plan_is_reported(prog, tmp_path):
    """the checker itself: a case whose validity flags break the engine's invariant (a valid vector over a stale input) is refused"""
    n = 5
    back = _full_back(trees.random_topology(n, np.random.default_rng(2)), n)
    valid = np.zeros(_records(n), dtype=np.int32)
    r = next(r for r in range(3 * (n + 1), 3 * (2 * n - 1)) if int(back[nx(r)]) // 3 > n)
    valid[r] = 1
    cs = Cases()
    cs.add(n, back, valid, None, None, None, 0)
    path = str(tmp_path / "bad.bin")
    with open(path, "wb") as f:
        for a in cs.blob:
            a.tofile(f)
    res = subprocess.run([prog, path], capture_output=True, text=True)
    assert res.returncode == 1 and "stale input" in res.stderr
