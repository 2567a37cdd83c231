"""The inputs of test_gpu_grow_edges.py are what they claim to be -- proved here from the oracle's own trees, without a device:
the closed form holds, the designed figure (fork depth, part count, root path, clusters at their depths) is there for the seeds
used, unsupported splits make ties that the tie stream decides, and the packing gives the row pitch and tile count of each case."""
import numpy as np
import pytest

import grow_cases as gc


def _ids(cases):
    return [c.name for c in cases]


FAST = [c for c in gc.all_cases() if c.n < 2049]              # (2049: the same shape one taxon on; its closed form runs on the device test)


def test_the_restated_addition_order_is_the_oracles():
    from oracle import pyoracle as po
    for n, seed in ((4, 5), (24, 17), (214, 21), (583, 11)):
        o = po.Oracle(np.ones((n, 1), dtype=np.uint8) << (np.arange(n)[:, None] % 2).astype(np.uint8))
        assert o.make_tree(seed, 0)[1][1:].tolist() == gc.addition_order(n, seed)


@pytest.mark.parametrize("c", FAST, ids=_ids(FAST))
def test_closed_form_design_and_start_tip(c):
    """(the 2048-taxon tree takes the oracle some seven seconds: its comparison is here, not in the device test)"""
    ref = gc.oracle_reference(c)
    assert c.start_tip == min(c.perm[:3]) and c.label_of_row[c.start_tip - 1] == 0
    assert ref["sites"] == c.nsites == c.codes.shape[1]
    assert ref["best"][4:] == c.closed[4:].tolist() and ref["score"] == c.closed[-1]
    got = gc.tree_splits(ref["tree"], c.n, c.start_tip)
    assert len(got) == c.n - 3
    if c.all_supported:
        assert got == c.design                                 # no tie can matter: the tree is the design
        if c.n < 1000:
            assert gc.oracle_reference(c, tie_seed=77)["tree"] == ref["tree"]
    else:
        assert c.design < got


OPEN = [c for c in FAST if c.open_splits]                      # (a cluster's inner splits are no such thing: the descent cut leaves one branch)


@pytest.mark.parametrize("c", OPEN, ids=_ids(OPEN))
def test_unsupported_splits_are_decided_by_the_tie_stream(c):
    ref = gc.oracle_reference(c)
    assert ref["tie_state"] != ref["seeded"]
    others = [gc.oracle_reference(c, tie_seed=s) for s in (101, 102, 103)]
    assert any(o["tree"] != ref["tree"] for o in others)       # a tie among the best branches, decided by a draw
    assert all(o["best"] == ref["best"] for o in others)


@pytest.mark.parametrize("depth", gc.DEPTHS)
def test_the_fork_sits_at_its_depth_in_the_trees_the_kernel_walks(depth):
    c = gc.depth_case(depth)
    ref = gc.oracle_reference(c)
    for nw in (16, 8):
        w = gc.walked_figures(ref["tree"], c.n, c.start_tip, nw, c.perm)
        f = gc.plan_figures((ref["tree"], c.n), c.start_tip, nw, c.perm[:c.n - 1])        # the last tree walked
        assert w.max_lev == f.max_lev == depth and f.S == {16: 24, 8: 48}[nw]
        assert f.nparts == 2 and f.max_path == depth + gc.FORK_TIPS[0] + 1      # (a fork child's deepest tip: 35 levels below the fork)
    assert (depth >= gc.PARK_SKEL) == (depth == 512)


def test_plan_figures_on_a_tree_small_enough_to_count_by_hand():
    """below the start tip ((1,2),((3,4),(5,(6,7)))): 13 nodes, S = 8.  The skeleton is the root and its child of 9 nodes; the parts
    are (1,2), (3,4) and (5,(6,7)); no skeleton node has both children walked; the deepest tips have four nodes above them"""
    n = 8
    c = gc._finish(gc._case("by hand", ((1, 2), ((3, 4), (5, (6, 7)))), n, seed=1, order=list(range(n))))
    ref = gc.oracle_reference(c)
    f = gc.plan_figures((ref["tree"], n), c.start_tip, 16)
    assert (f.m, f.S, f.nskel, f.nparts, f.max_lev, f.max_path) == (13, 8, 2, 3, -1, 5)
    # ... and with S forced below every subtree by a cut-down tree: five taxa -> m = 7 <= S: one part, no skeleton
    g = gc.plan_figures((ref["tree"], n), c.start_tip, 16, c.perm[:5])
    assert (g.m, g.nskel, g.nparts) == (7, 0, 1)


def test_part_count_of_the_cherry_caterpillar_at_the_size_bound():
    c = gc.size_case(2048)
    ref = gc.oracle_reference(c)
    for nw in (16, 8):
        w = gc.walked_figures(ref["tree"], c.n, c.start_tip, nw, c.perm, stride=8)
        assert w.nparts == 1008 <= gc.MAX_PARTS and w.max_lev == -1 and w.max_path == 1025
    ce, Wp = gc.packing(c.nsites)
    assert (ce, Wp, gc.tiles_of(Wp, 4), gc.tiles_of(Wp, 1)) == (64, 64, 1, 4)
    assert 2 * c.n - 3 == 4093 <= 8 * 512                      # entries step (6) moves, eight per thread of an 8-wave workgroup


@pytest.mark.parametrize("variant", gc.CUT_VARIANTS)
def test_clusters_sit_either_side_of_the_ballot_chunks(variant):
    c = gc.cut_case(variant)
    ref = gc.oracle_reference(c)
    R = gc.Rooted(ref["tree"], c.n, c.start_tip)
    depths = []
    for k, cl in enumerate(c.clusters):
        is_clade, depth, _ = gc.clade(R, cl)
        rows = c.codes[np.array(cl) - 1]
        assert is_clade and 3 <= len(cl) <= 6
        assert (rows == rows[0]).all() == (k != c.costly)      # identical taxa: the subtree costs nothing
        depths.append(depth)
    for lo, hi in ((48, 64), (64, 80), (80, 128), (128, 144)):
        assert any(lo <= d < hi for d in depths), (depths, lo, hi)
    for nw in (16, 8):
        assert gc.walked_figures(ref["tree"], c.n, c.start_tip, nw, c.perm).max_path > 128       # root paths of three ballot chunks
    ce, Wp = gc.packing(c.nsites)
    assert (ce, Wp) == (150, 160) and c.nsites % 32 == {"plain": 29, "last partial word": 1}.get(variant, 0)
    assert {t: gc.tiles_of(Wp, t) for t in gc.DNA_TILES} == gc.CUT_TILES
    for t in gc.DNA_TILES:                                     # the last live word lies in every shape's last tile
        assert (ce - 1) // gc.grow_shape(t)[0] == gc.CUT_TILES[t] - 1
    if variant != "plain":
        col = int(np.nonzero((c.codes[np.array(c.clusters[c.costly]) - 1] != c.codes[c.clusters[c.costly][0] - 1]).any(axis=0))[0][0])
        assert col // 32 == {"first word": 0, "last word of the last tile": ce - 1, "last partial word": ce - 1}[variant]
        a, b = [c.perm.index(t) for t in c.clusters[c.costly]][1:3]
        first = min(c.perm.index(t) for t in c.clusters[c.costly])
        assert first == a < b                                   # the differing pair: first and third of its cluster


def test_the_early_cluster():
    c = gc.early_cluster_case(8)
    ref = gc.oracle_reference(c)
    cl = c.clusters[0]
    at = sorted(c.perm.index(t) for t in cl)
    assert at[0] in (0, 1) and at[1:] == [3, 4]                # one of the start tree's taxa, then the first two taxa added
    rows = c.codes[np.array(cl) - 1]
    assert (rows == rows[0]).all()
    first3 = c.codes[np.array(c.perm[:3]) - 1]
    assert len({r.tobytes() for r in first3}) == 3             # the start tree costs something
    assert gc.clade(gc.Rooted(ref["tree"], c.n, c.start_tip), cl)[0]


def test_the_homoplasy_case_has_homoplasy():
    for dt, rows in ((gc.DNA, 4), (gc.AA, 20), (gc.GENERIC, 32)):
        c = gc.noisy_case(dt)
        ref = gc.oracle_reference(c)
        assert ref["score"] > c.closed[-1] + 48 and ref["rows"] == rows      # every such column costs two steps at least
        assert gc.packing(ref["sites"]) == (32, 32) and ref["sites"] % 32 == 17
        assert ref["tie_state"] != ref["seeded"]


def _tail_splits_live_in_the_last_word_only(c):
    part = c.codes == c.codes[0:1]                              # a two-state column's split
    last = (c.nsites - 1) // 32 * 32
    tail = {part[:, j].tobytes() for j in range(last, c.nsites)}
    assert 1 <= len(tail) <= 3
    assert not any(part[:, j].tobytes() in tail for j in range(last))


@pytest.mark.parametrize("rem", gc.REMS)
def test_row_tail_packing(rem):
    for Wp in (32, 96, 160):
        c = gc.tail_case(Wp, rem)
        ref = gc.oracle_reference(c)
        assert gc.packing(ref["sites"]) == (Wp, Wp) and ref["sites"] % 32 == rem and ref["rows"] == 4       # (live words = row pitch)
        _tail_splits_live_in_the_last_word_only(c)
        for t, wp, tiles in gc.TAIL_DNA:
            if wp == Wp:
                assert gc.tiles_of(Wp, t) == tiles
    for dt, Wp, tiles in gc.TAIL_OTHER:
        c = gc.tail_case(Wp, rem, dt)
        ref = gc.oracle_reference(c)
        assert gc.packing(ref["sites"]) == (Wp, Wp) and ref["sites"] % 32 == rem and ref["rows"] == {gc.AA: 20, gc.GENERIC: 32}[dt]
        assert gc.tiles_of(Wp, None, dt) == tiles
