"""The shape rule of a round of mpf_optimize_spr_many_round (mpboot_amd/host/many_shape.hpp: which active climbs form the launch of
k_climb_many, on what tile width / states / word-major flag / device, and which run alone) as a stand-alone program built with
-fsanitize=address,undefined (mpboot_amd/host/many_shape_main.cpp).  No GPU, nothing loaded into python: the program runs as a
child process over a table of cases and prints one line per case; any output on stderr fails the test.

The program also evaluates the rule this one replaced -- "the launch takes the shape of the first active engine, only starting climbs
are compared with it" -- and reports how many continuing climbs that rule would have launched on a width they were not laid out for.
The case `starter_at_0_beside_continuing` is the counter-example: a finished engine at index 0, re-weighted across a row-pitch
boundary (64 -> 96 words: 64-word tiles -> 32-word tiles) and started beside three climbs that go on."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

SRC = os.path.join(ROOT, "mpboot_amd", "host", "many_shape_main.cpp")
MPF_E_STATE = -5


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed")
    exe = str(tmp_path_factory.mktemp("many_shape") / "many_shape")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", SRC, "-o", exe])
    return exe


# shapes: (vw, S, dev, wm).  DNA rows of an even multiple of 32 words fit 64-word tiles word-major, odd multiples 32-word tiles
W4 = (4, 4, 0, 1)
W2 = (2, 4, 0, 0)
AA = (1, 20, 0, 0)
NONE = (0, 4, 0, 0)          # no width fits (the weighted engine, an alignment too long for one workgroup)
DEV1 = (4, 4, 1, 1)


def start(shape, fits=1, gen=5):
    return (1,) + shape + (gen, fits) + (0, 0, 0, 0, 0)


def cont(shape, gen=5, now=None, now_gen=None):
    return (2,) + (now or shape) + (gen if now_gen is None else now_gen, 1) + shape + (gen,)


IDLE = (0,) * 12


def want(rc=0, shape=None, batch=(), alone=(), parent_vw=None, parent_batch=None, foreign=0):
    return dict(rc=rc, shape=shape, batch=list(batch), alone=list(alone), parent_vw=parent_vw, parent_batch=parent_batch, foreign=foreign)


CASES = {
    "empty": ([], want()),
    "nobody_active": ([IDLE, IDLE], want()),
    "single_starter": ([start(W4)], want(shape=W4, batch=[0], parent_vw=4, parent_batch=[0])),
    "single_misfit": ([start(W4, fits=0)], want(alone=[0])),
    "single_continuing": ([IDLE, cont(W2)], want(shape=W2, batch=[1], parent_vw=2, parent_batch=[1])),
    "all_start_equal": ([start(W4), start(W4, gen=9), start(W4)], want(shape=W4, batch=[0, 1, 2], parent_vw=4, parent_batch=[0, 1, 2])),
    "mismatched_starter_at_a_higher_index": ([start(W4), start(W4), IDLE, start(W2)], want(shape=W4, batch=[0, 1], alone=[3], parent_vw=4, parent_batch=[0, 1])),
    # the defect: the parent's rule launches the three continuing 64-word-tile climbs on engine 0's 32-word tiles
    "starter_at_0_beside_continuing": ([start(W2, gen=8), cont(W4), cont(W4), cont(W4)],
                                       want(shape=W4, batch=[1, 2, 3], alone=[0], parent_vw=2, parent_batch=[0, 1, 2, 3], foreign=3)),
    # ... and the other direction: 32-word-tile climbs launched on 64-word tiles would read beyond their 96-word rows
    "wide_starter_at_0_beside_narrow_continuing": ([start(W4, gen=8), IDLE, cont(W2), cont(W2)],
                                                   want(shape=W2, batch=[2, 3], alone=[0], parent_vw=4, parent_batch=[0, 2, 3], foreign=2)),
    "matching_starter_joins_continuing": ([start(W4), cont(W4), start(W2), start(W4)], want(shape=W4, batch=[0, 1, 3], alone=[2], parent_vw=4, parent_batch=[0, 1, 3])),
    "continuing_disagree": ([cont(W4), cont(W2)], want(rc=MPF_E_STATE, parent_vw=4, parent_batch=[0, 1], foreign=1)),
    "continuing_disagree_on_word_major": ([cont(W4), cont((4, 4, 0, 0))], want(rc=MPF_E_STATE, parent_vw=4, parent_batch=[0, 1], foreign=1)),
    "continuing_repacked": ([cont(W4), cont(W4, gen=5, now_gen=6)], want(rc=MPF_E_STATE, parent_vw=4, parent_batch=[0, 1])),
    "continuing_repacked_across_a_pitch": ([cont(W4, gen=5, now=W2, now_gen=6), cont(W4)], want(rc=MPF_E_STATE, parent_vw=2, parent_batch=[0, 1], foreign=2)),
    "continuing_option_changed": ([start(W4), cont(W4, now=(1, 4, 0, 0))], want(rc=MPF_E_STATE, parent_vw=4, parent_batch=[0, 1])),
    "continuing_never_started": ([(2,) + W4 + (5, 1) + (0, 0, 0, 0, 0)], want(rc=MPF_E_STATE, parent_vw=4, parent_batch=[0], foreign=1)),
    # the first active engine cannot join (the weighted engine: no width; a tracker attached: fits 0; protein beside DNA)
    "first_active_weighted_others_continue": ([start(NONE, fits=0), cont(W4), cont(W4)], want(shape=W4, batch=[1, 2], alone=[0], parent_vw=0, parent_batch=[1, 2], foreign=2)),
    "first_active_tracked_others_continue": ([IDLE, start(W4, fits=0), cont(W4), start(W4)], want(shape=W4, batch=[2, 3], alone=[1], parent_vw=4, parent_batch=[2, 3])),
    "first_active_other_alphabet_others_continue": ([start(AA), cont(W4), start(W4)], want(shape=W4, batch=[1, 2], alone=[0], parent_vw=1, parent_batch=[0, 1], foreign=1)),
    "first_starter_misfit_second_gives_the_shape": ([start(W2, fits=0), start(W4), start(W2), start(W4)], want(shape=W4, batch=[1, 3], alone=[0, 2], parent_vw=2, parent_batch=[2])),
    "other_device_runs_alone": ([start(W4), start(DEV1), start(W4)], want(shape=W4, batch=[0, 2], alone=[1], parent_vw=4, parent_batch=[0, 2])),
    "nobody_fits": ([start(NONE, fits=0), start(W4, fits=0)], want(alone=[0, 1])),
}


def _parse(line):
    head, parent = [x.strip() for x in line.split("|")[:2]]
    tok = head.split()
    got = dict(zip(tok[2::2], tok[3::2]))
    ptok = parent.split()
    assert ptok[0] == "parent"
    got.update({"parent_" + k: v for k, v in zip(ptok[1::2], ptok[2::2])})
    ints = lambda s: [] if s == "-" else [int(x) for x in s.split(",")]   # noqa: E731
    return dict(rc=int(got["rc"]), shape=(int(got["vw"]), int(got["S"]), int(got["dev"]), int(got["wm"])), batch=ints(got["batch"]), alone=ints(got["alone"]),
                owner=int(got["owner"]), parent_vw=int(got["parent_vw"]), parent_batch=ints(got["parent_batch"]), foreign=int(got["parent_foreign"]),
                message=line.split("|")[2].strip() if line.count("|") >= 2 else "")


@pytest.fixture(scope="module")
def results(prog, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("many_shape_cases") / "cases.txt")
    with open(path, "w") as f:
        for entries, _w in CASES.values():
            f.write(" ".join([str(len(entries))] + [str(int(x)) for e in entries for x in e]) + "\n")
    r = subprocess.run([prog, path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    for i, line in enumerate(lines):
        assert line.split()[:2] == ["case", str(i)]
    return dict(zip(CASES, (_parse(x) for x in lines)))


@pytest.mark.parametrize("name", list(CASES))
def test_shape_rule(results, name):
    entries, w = CASES[name]
    got = results[name]
    assert got["rc"] == w["rc"], got
    if w["rc"]:
        assert got["message"] and got["batch"] == [] and got["alone"] == [], got
    else:
        assert got["batch"] == w["batch"] and got["alone"] == w["alone"], got
        assert got["owner"] == (w["batch"][0] if w["batch"] else -1), got
        assert got["shape"] == ((w["shape"][0], w["shape"][1], w["shape"][2], w["shape"][3]) if w["batch"] else (0, 0, 0, 0)), got
    if w["parent_vw"] is not None:
        assert got["parent_vw"] == w["parent_vw"] and got["parent_batch"] == w["parent_batch"], got
    assert got["foreign"] == w["foreign"], got


def test_the_replaced_rule_hands_continuing_climbs_a_foreign_width(results):
    """the executable counter-example: engine 0 starts on 32-word tiles beside three climbs laid out for 64-word word-major tiles.  The
    replaced rule takes engine 0's shape for the launch and puts all four into it; the rule in force keeps the continuing climbs'
    shape and runs engine 0 alone."""
    got = results["starter_at_0_beside_continuing"]
    entries, _w = CASES["starter_at_0_beside_continuing"]
    continuing = [k for k, e in enumerate(entries) if e[0] == 2]
    assert continuing == [1, 2, 3]
    assert set(continuing) <= set(got["parent_batch"]) and got["parent_vw"] == 2
    assert all(entries[k][7] != got["parent_vw"] for k in continuing) and got["foreign"] == len(continuing)
    assert got["rc"] == 0 and got["shape"] == W4 and got["batch"] == continuing and got["alone"] == [0]
    # the other direction reads beyond the rows
    got = results["wide_starter_at_0_beside_narrow_continuing"]
    assert got["parent_vw"] == 4 and got["foreign"] == 2 and got["shape"] == W2 and got["alone"] == [0]


def test_a_wrong_case_line_is_refused(prog, tmp_path):
    path = str(tmp_path / "bad.txt")
    with open(path, "w") as f:
        f.write("2 1 4 4 0 1 5 1 0 0 0 0 0\n")          # two engines announced, one given
    r = subprocess.run([prog, path], capture_output=True, text=True)
    assert r.returncode == 2 and "short case line" in r.stderr
