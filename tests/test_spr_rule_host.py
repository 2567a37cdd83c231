"""The two rules every SPR sweep loop decides by (mpboot_amd/host/spr_rule.hpp: testInsertParsimony's tie rule and the sweep's
accept rule) as a stand-alone program built with -fsanitize=address,undefined, against a plain restatement of the reference's
lines with mpboot_amd.rng.Lcg64 for the draws.  Every visit's line is compared, the generator's state included: that pins the
number of draws exactly.  No GPU, nothing loaded into python: the program runs as a child process and a sanitizer report fails
the run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from mpboot_amd.rng import Lcg64

SRC = os.path.join(ROOT, "mpboot_amd", "host", "spr_rule_main.cpp")
TIE_FIRST, TIE_RANDOM = 0, 1                   # include/mpfitch.h
MODES = (TIE_FIRST, TIE_RANDOM)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("spr_rule") / "spr_rule")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


class Reference:
    """pllOptimizeSprParsimony's loop body around rearrangeParsimony, reduced to what it decides (sprparsimony.cpp)"""

    def __init__(self, tie_mode, seed, best, random_mp):
        self.random = tie_mode == TIE_RANDOM
        self.rng = Lcg64(seed)
        self.best, self.random_mp = best, random_mp
        self.hits = 1                          # bestTreeScoreHits
        self.iter_hits = 1                     # bestIterationScoreHits, :3292

    def draw(self):
        return float(self.rng.doubles(1)[0])   # random_double()

    def visit(self, have_move, costs):
        if self.random:
            self.hits = 1                                                                   # :3303
        taken = -1
        for c, mp in enumerate(costs):                                                      # testInsertParsimony, one per candidate
            if self.random:
                if mp < self.best:                                                          # :2168
                    self.hits = 1
                elif mp == self.best:                                                       # :2169
                    self.hits += 1
                if mp < self.best or (mp == self.best and self.draw() <= 1.0 / self.hits):  # :2171-2172
                    self.best, taken = mp, c                                                # :2173-2175
            elif mp < self.best:                                                            # strict '<' (fastDNAparsimony.c:1224-1229)
                self.best, taken = mp, c
        if self.random:
            if self.best == self.random_mp:                                                 # :3306
                self.iter_hits += 1
            if self.best < self.random_mp:                                                  # :3307
                self.iter_hits = 1
            accept = bool((self.best < self.random_mp or                                    # :3308-3311: the draw, then the move test
                           (self.best == self.random_mp and self.draw() <= 1.0 / self.iter_hits)) and have_move)
        else:
            accept = self.best < self.random_mp
        if accept:
            self.random_mp = self.best                                                      # :3313
        return "%d %d %d %d %d %016x" % (taken, self.best, self.hits, self.iter_hits, int(accept), int(self.rng.state))


def _run(prog, tie_mode, seed, best, random_mp, visits):
    """the program's lines and the restatement's; visits: (have_move, costs)"""
    assert len(visits) <= 20 and all(len(c) <= 8 for _, c in visits)
    text = "%d %d %d %d %d\n" % (tie_mode, seed, best, random_mp, len(visits))
    text += "".join("%d %d %s\n" % (int(m), len(c), " ".join(str(int(x)) for x in c)) for m, c in visits)
    res = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    ref = Reference(tie_mode, seed, best, random_mp)
    return res.stdout.splitlines(), [ref.visit(m, c) for m, c in visits]


def _state(seed, draws):
    """the generator's state behind so many draws"""
    g = Lcg64(seed)
    g.doubles(draws)
    return "%016x" % int(g.state)


def _fields(line):
    taken, best, hits, iter_hits, accept, state = line.split()
    return int(taken), int(best), int(hits), int(iter_hits), int(accept), state


@pytest.mark.parametrize("tie_mode", MODES)
def test_visit_without_a_candidate(prog, tie_mode):
    got, want = _run(prog, tie_mode, 3, 100, 100, [(0, []), (1, []), (0, [])])
    assert got == want
    for v, line in enumerate(got):
        # random: one accept draw per visit and a hit of the iteration, nothing selected; first-best: nothing at all
        assert _fields(line) == ((-1, 100, 1, v + 2, _fields(line)[4], _state(3, v + 1)) if tie_mode == TIE_RANDOM else (-1, 100, 1, 1, 0, _state(3, 0)))
    # (without a move the draw's outcome is void)
    assert _fields(got[0])[4] == 0 and _fields(got[2])[4] == 0


@pytest.mark.parametrize("tie_mode", MODES)
def test_all_candidates_worse(prog, tie_mode):
    got, want = _run(prog, tie_mode, 4, 100, 100, [(1, [101, 150, 101, 4000000000]), (1, [102] * 8)])
    assert got == want
    # no draw inside the visit: what is drawn is the accept rule's one draw per visit (random mode)
    assert [_fields(x)[5] for x in got] == [_state(4, v + 1 if tie_mode == TIE_RANDOM else 0) for v in range(2)]
    assert all(_fields(x)[:3] == (-1, 100, 1) for x in got)


@pytest.mark.parametrize("tie_mode", MODES)
def test_all_candidates_equal(prog, tie_mode):
    got, want = _run(prog, tie_mode, 5, 100, 100, [(1, [100] * 8), (0, [100] * 3), (1, [100])])
    assert got == want
    if tie_mode == TIE_RANDOM:
        # a draw each, hits running 2, 3, ..: k + 1 behind the visit; k + 1 draws with the accept rule's
        assert [_fields(x)[2] for x in got] == [9, 4, 2]
        assert [_fields(x)[5] for x in got] == [_state(5, 9), _state(5, 13), _state(5, 15)]
        assert _fields(got[1])[4] == 0
    else:
        assert all(_fields(x) == (-1, 100, 1, 1, 0, _state(5, 0)) for x in got)


@pytest.mark.parametrize("tie_mode", MODES)
def test_better_candidate_behind_ties(prog, tie_mode):
    got, want = _run(prog, tie_mode, 6, 100, 100, [(1, [100, 100, 99, 99, 101, 99]), (1, [99, 98])])
    assert got == want
    taken, best, hits, iter_hits, accept, state = _fields(got[0])
    if tie_mode == TIE_RANDOM:
        # two ties drawn, 99 taken without a draw and the hits back to 1, two ties with the new best drawn; accepted without a draw
        assert (best, hits, iter_hits, accept, state) == (99, 3, 1, 1, _state(6, 4)) and taken in (2, 3, 5)
        assert _fields(got[1])[:5] == (1, 98, 1, 1, 1) and _fields(got[1])[5] == _state(6, 5)
    else:
        assert (taken, best, accept, state) == (2, 99, 1, _state(6, 0)) and _fields(got[1])[:2] == (1, 98)


@pytest.mark.parametrize("tie_mode", MODES)
@pytest.mark.parametrize("have_move", (0, 1))
def test_level_with_the_current_tree(prog, tie_mode, have_move):
    visits = [(have_move, [100, 101])] * 20
    got, want = _run(prog, tie_mode, 7, 100, 100, visits)
    assert got == want
    if tie_mode == TIE_RANDOM:
        # two draws per visit whether a move can be selected or not; accepted only with one
        assert [_fields(x)[5] for x in got] == [_state(7, 2 * (v + 1)) for v in range(20)]
        assert [_fields(x)[3] for x in got] == list(range(2, 22))
        second = Lcg64(7).doubles(40)[1::2]                    # the accept rule's draw of every visit, against 1 / iter_hits
        assert [_fields(x)[4] for x in got] == [int(bool(have_move) and second[v] <= 1.0 / (v + 2)) for v in range(20)]
    else:
        assert all(_fields(x)[4] == 0 for x in got)


@pytest.mark.parametrize("tie_mode", MODES)
@pytest.mark.parametrize("have_move", (0, 1))
def test_better_than_the_current_tree(prog, tie_mode, have_move):
    got, want = _run(prog, tie_mode, 8, 95, 100, [(have_move, []), (have_move, [97, 95, 94])])
    assert got == want
    # no draw; the iteration's hits start again; the random rule wants a move, the first-best rule asks for none
    assert _fields(got[0]) == (-1, 95, 1, 1, int(have_move or tie_mode == TIE_FIRST), _state(8, 0))
    assert _fields(got[1])[:2] == (2, 94)


@pytest.mark.parametrize("tie_mode", MODES)
def test_random_visits_with_frequent_ties(prog, tie_mode):
    rng = np.random.default_rng(11 + tie_mode)
    n_visits = 0
    for stream in range(16):
        base = int(rng.integers(1, 1000))
        start = base + int(rng.integers(1, 3))
        visits = [(int(rng.integers(0, 2)), (base + rng.integers(0, 3, size=int(rng.integers(0, 9)))).tolist()) for _ in range(20)]
        got, want = _run(prog, tie_mode, stream - 3, start, start, visits)
        assert got == want, stream
        n_visits += len(visits)
    assert n_visits == 320
