"""The one walk that checks a tree's back links and lays out the topology array the device reads (mpboot_amd/host/tree_links.hpp,
the code Engine::set_tree and Engine::schedule_views_dev run), WITHOUT a GPU and under the address and undefined-behaviour
sanitizers: tests/cpu/tree_links_test.cpp compares the layout of random topologies with a plain restatement of the two loops the
walk replaced, and hands it the corruptions it has to reject -- with arrays of exactly the documented sizes, so that a read or a
write past them is reported."""
import os
import subprocess

import pytest

from helpers import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "tree_links_test.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tree_links") / "tree_links_test")
    base = ["g++", "-std=c++17", "-O1", "-g", SRC, "-o", out]
    r = subprocess.run(base[:4] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + base[4:], capture_output=True, text=True)
    san = r.returncode == 0
    if not san:                                    # (a toolchain without the sanitizers' runtime: the comparison still runs)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out, san


def _run(prog, *args):
    r = subprocess.run([prog[0], *args], capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def test_sanitizers_are_in_the_build(prog):
    assert prog[1], "g++ -fsanitize=address,undefined did not build here"


def test_layout_equals_the_plain_loops(prog):
    out = _run(prog, "layout", "7", "2000")
    assert "2000 layouts equal" in out and "DIFFERENT" not in out


def test_corrupted_links_are_rejected(prog):
    out = _run(prog, "reject", "11", "500")
    assert "ACCEPTED" not in out
    assert "rejected: below-3 500, past-the-end 500, one-way 500, tip-unused 500" in out
