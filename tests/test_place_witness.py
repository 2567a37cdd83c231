"""CPU checks of the taxon-insertion witness (tests/place_witness.py) against the pinned oracle: on the golden alignments the length
of a tree with one taxon dropped and attached to every branch equals Oracle.score_tree of the completed tree, the witness's stepwise
tree has the length the oracle gives it, and the witness's two forms agree.  No GPU."""
import numpy as np
import pytest

import place_witness as plw
from helpers import load_fixture
from mpboot_amd import trees
from mpboot_amd.rng import Lcg64
from oracle import pyoracle as po

GOLDEN = ("dna_ambig", "aa", "bin", "morph32")          # DNA with ambiguity, protein, binary, the 32-symbol alphabet


def _fixture(name, keep_all):
    fx = load_fixture(name)
    codes, weights, dt = fx["codes_np"], fx["weights_np"], fx["datatype"]
    orc = po.Oracle(codes, weights, datatype=dt, keep_all=keep_all)
    wit = plw.PlaceWitness(codes, weights, dt, keep=None if keep_all else orc.informative())
    return codes.shape[0], orc, wit


@pytest.mark.parametrize("keep_all", [False, True], ids=["informative", "keep_all"])
@pytest.mark.parametrize("name", GOLDEN)
def test_every_attachment_has_the_oracles_length(name, keep_all):
    n, orc, wit = _fixture(name, keep_all)
    rng = np.random.default_rng(len(name))
    back = trees.random_topology(n, rng)
    for t in (int(rng.integers(2, n + 1)), 1):
        root = 1 if t != 1 else 2
        first, nbr = trees.drop_tips(back, n, [t])
        assert plw.check(first, nbr, n, root) == "ok"
        br, cost = wit.costs(first, nbr, [t], root)
        assert len(br) == 2 * (n - 1) - 3
        vbr, vcost, vlen = wit.view_costs(first, nbr, [t], root)
        assert vbr == br and (vcost == cost).all() and vlen == wit.length(first, nbr, root)
        for i, (a, b) in enumerate(br):
            f2, n2 = trees.insert_tip(first, nbr, n, t, a, b)
            assert int(cost[0, i]) == orc.score_tree(trees.lists_to_back(f2, n2, n)), (t, a, b)
        # one of the attachments is the tree the taxon came from
        assert orc.score_tree(back) in cost[0].tolist()


@pytest.mark.parametrize("name", GOLDEN)
def test_the_stepwise_tree_has_the_oracles_length(name):
    n, orc, wit = _fixture(name, False)
    order = plw.shuffle(n, Lcg64(7))
    assert sorted(order) == list(range(1, n + 1))
    first, nbr, lengths = plw.stepwise(wit, order)
    assert len(lengths) == n - 2 and lengths == sorted(lengths)
    assert plw.check(first, nbr, n, order[0]) == "ok" and len(first) == n - 1
    assert list(first[:2]) == [0, 3]
    assert lengths[-1] == orc.score_tree(trees.lists_to_back(first, nbr, n))
    # the node made last still lists its taxon first (earlier ones may have been rewired by later insertions)
    assert nbr[-3] == order[-1]


def test_the_two_forms_agree_on_small_backbones():
    rng = np.random.default_rng(5)
    for n, P, dt in ((4, 9, 0), (5, 7, 1), (6, 5, 3), (9, 33, 0), (12, 6, 1)):
        hi = {0: 16, 1: 23, 3: 33}[dt]
        codes = rng.integers(1 if dt == 0 else 0, hi, size=(n, P)).astype(np.uint8)
        wit = plw.PlaceWitness(codes, rng.integers(1, 6, size=P), dt)
        for m in range(3, n):
            tips = rng.permutation(n)[:m] + 1
            first, nbr = plw.backbone(n, tips, rng)
            rest = [t for t in range(1, n + 1) if t not in tips.tolist()]
            for root in tips.tolist():
                br, cost = wit.costs(first, nbr, rest, root)
                vbr, vcost, vlen = wit.view_costs(first, nbr, rest, root)
                assert br == vbr == plw.walk(first, nbr, n, root) and (cost == vcost).all() and vlen == wit.length(first, nbr, root)
                assert len(br) == 2 * m - 3 and br[0][0] == root


def test_check_first_minimum_and_helpers():
    assert plw.check(*plw.GOOD, 9, 1) == "ok" and plw.check(*plw.GOOD, 9, 5) == "ok"
    for name, (first, nbr, root, verdict) in plw.MALFORMED.items():
        assert plw.check(first, nbr, 9, root) == verdict, name
    assert plw.first_min([5, 3, 4, 3, 3]) == 1 and plw.first_min([2]) == 0 and plw.first_min([4, 4]) == 0
    # the walk of the good backbone from tip 1 and from tip 5: the tie order changes with the root
    assert plw.walk(*plw.GOOD, 9, 1) == [(1, 10), (10, 2), (10, 11), (11, 3), (11, 12), (12, 4), (12, 5)]
    assert plw.walk(*plw.GOOD, 9, 5)[:3] == [(5, 12), (12, 11), (11, 10)]
    # trees.insert_tip is the witness's rewiring; drop_tips undoes it up to numbering
    f, nb = plw.grow(*plw.GOOD, 9, 7, 11, 12)
    f2, nb2 = trees.insert_tip(*plw.GOOD, 9, 7, 11, 12)
    assert f == f2.tolist() and nb == nb2.tolist() and nb[-3:] == [7, 12, 11]
    assert nb[3:6] == [10, 3, 13] and nb[6:9] == [13, 4, 5]
    g, gb = trees.drop_tips((f2, nb2), 9, [7])
    assert g.tolist() == plw.GOOD[0] and gb.tolist() == plw.GOOD[1]
