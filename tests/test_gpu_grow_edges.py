"""k_grow at the edges of its plan (csrc/grow.hip): the depth bound of the skeleton's parked vectors (kGrowParkSkel), the size bound of
grow_supported and the part list, the descent cut's flags over root paths longer than a ballot and over several tiles, and the row
tails of every lane shape.  The inputs have a designed tree (grow_cases.py; test_grow_cases_host.py proves each one's figure from
the oracle's tree).  Every case compares the kernel with the host-driven loop and with the oracle -- per-step lengths, insertion
branches, tree, score, state of the tie stream, all exact -- and asserts grow_launches / grow_last_err: the path taken is known."""
import pytest

import grow_cases as gc

pytestmark = pytest.mark.gpu

_HOST = {}


def _run(c, dev, tile=None):
    from mpboot_amd import engine
    e = engine.FitchEngine(c.codes, datatype=c.datatype)
    if tile is not None:
        e.set_option("grow_tile", tile)
    e.set_option("grow_device", dev)
    e.seed_ties(engine.TIE_RANDOM, c.tie_seed)
    return e, _add(e, c)


def _add(e, c):
    score, best, ins = e.stepwise_addition(c.seed)
    return dict(score=score, best=best.tolist(), ins=ins.tolist(), tree=e.get_tree().tolist(), tie_state=e.tie_state())


def _host(c):
    """the host-driven loop's result for a case, computed once"""
    if c.name not in _HOST:
        e, _HOST[c.name] = _run(c, 0)
        assert e.get_option("grow_launches") == 0
    return _HOST[c.name]


def _oracle(c):
    ref = gc.oracle_reference(c)
    return {k: ref[k] for k in ("score", "best", "ins", "tree", "tie_state")}


def _closed_form(c, got):
    assert got["best"][4:] == c.closed[4:].tolist() and got["score"] == c.closed[-1]
    splits = gc.tree_splits(got["tree"], c.n, c.start_tip)
    assert splits == c.design if c.all_supported else c.design < splits


def _kernel_built_it(e, launches=1):
    assert (e.get_option("grow_launches"), e.get_option("grow_last_err")) == (launches, 0)


# ---- A. depth
_FOLLOW = {}


def _oracle_follow_up(c):
    """the oracle's score and one SPR climb behind the tree of a case"""
    if c.name not in _FOLLOW:
        from oracle import pyoracle as po
        o = po.Oracle(c.codes, datatype=c.datatype)
        o.seed_ties(po.TIE_RANDOM, c.tie_seed)
        o.stepwise(c.seed)
        length = o.score_tree()
        o.seed_ties(po.TIE_RANDOM, 9)
        _FOLLOW[c.name] = (length, o.optimize_spr(1, 6), o.get_tree().tolist(), o.tie_state())
    return _FOLLOW[c.name]


@pytest.mark.parametrize("tile", [1, 4])
@pytest.mark.parametrize("depth", gc.DEPTHS)
def test_fork_at_the_depth_bound(depth, tile):
    """a node with both children walked parks its second child's U at level dep - dep(root): 511 is the last level there is, at 512
    the kernel reports GROW_ERROR 3 (grow_last_err 503) and the host's loop builds the tree.  16-wave (tile 1) and 8-wave shape."""
    from mpboot_amd import engine
    c = gc.depth_case(depth)
    ref = _oracle(c)
    w = gc.walked_figures(ref["tree"], c.n, c.start_tip, gc.grow_shape(tile)[1], c.perm)
    assert w.max_lev == depth                                   # (plan_figures off by one: this or the error below fails for one of the pair)
    e, got = _run(c, 1, tile)
    assert e.Wp == 32 and gc.tiles_of(e.Wp, tile) == {1: 2, 4: 1}[tile]
    assert got == _host(c) == ref
    _closed_form(c, got)
    if w.max_lev < gc.PARK_SKEL:
        _kernel_built_it(e)
        return
    assert (e.get_option("grow_launches"), e.get_option("grow_last_err"), e.get_option("grow_steps")) == (1, 503, 0)
    e.seed_ties(engine.TIE_RANDOM, c.tie_seed)
    assert _add(e, c) == ref                                    # the next tree on this engine: the same way out
    assert (e.get_option("grow_launches"), e.get_option("grow_last_err"), e.get_option("grow_steps")) == (2, 503, 0)
    length, climbed, tree, state = _oracle_follow_up(c)
    assert e.score_tree() == length == ref["score"]
    e.seed_ties(engine.TIE_RANDOM, 9)
    assert e.optimize_spr(1, 6) == climbed
    assert e.get_tree().tolist() == tree and e.tie_state() == state


# ---- B. size
@pytest.mark.parametrize("tile", [4, 1])
def test_cherry_caterpillar_at_the_size_bound(tile):
    """n = 2048: m = 4093 of the 4096 entries step (6) can move (tile 4, 8 waves: all eight per thread), 140 KB of LDS, and the
    shape that leaves most parts: 1008 of kGrowMaxParts = 1024.  Against the closed form and the host's loop (the oracle takes
    seven seconds for this tree: test_grow_cases_host.py compares it with the same closed form)."""
    c = gc.size_case(2048)
    e, got = _run(c, 1, tile)
    _kernel_built_it(e)
    assert e.Wp == 64 and gc.tiles_of(e.Wp, tile) == {4: 1, 1: 4}[tile]
    _closed_form(c, got)
    assert got == _host(c)
    w = gc.walked_figures(got["tree"], c.n, c.start_tip, gc.grow_shape(tile)[1], c.perm, stride=8)
    assert w.nparts == 1008 <= gc.MAX_PARTS


def test_one_taxon_past_the_size_bound_is_the_hosts():
    c = gc.size_case(2049)
    e, got = _run(c, 1, 4)
    _kernel_built_it(e, launches=0)
    _closed_form(c, got)


@pytest.mark.parametrize("n", [4, 5])
def test_one_and_two_steps(n):
    """no skeleton, one part; the fitted tile, the word-major layout and the widest tile (a quarter of one tile live)"""
    c = gc.size_case(n)
    for tile in (None, 0, 8):
        e, got = _run(c, 1, tile)
        _kernel_built_it(e)
        assert got == _host(c) == _oracle(c)
        _closed_form(c, got)


# ---- C. descent cut
@pytest.mark.parametrize("tile", gc.DNA_TILES)
@pytest.mark.parametrize("variant", gc.CUT_VARIANTS)
def test_descent_cut_over_long_paths_and_tiles(variant, tile):
    """214 taxa, clusters of identical taxa at depths either side of 64 and 128, root paths of three ballot chunks, 45 branches that
    ties decide; Wp = 160, the last live word in the last of 2 .. 10 tiles.  Variants: one cluster's subtree costs something at
    ONE site -- in the first word, in the last live word, alone in the last partial word: it must be descended into."""
    c = gc.cut_case(variant)
    e, got = _run(c, 1, tile)
    _kernel_built_it(e)
    assert e.Wp == 160 and gc.tiles_of(e.Wp, tile) == gc.CUT_TILES[tile] and e.num_informative % 32 == c.nsites % 32
    assert got == _host(c) == _oracle(c)
    _closed_form(c, got)


@pytest.mark.parametrize("tile", gc.DNA_TILES)
def test_first_root_path_entry_counts_as_not_zero_before(tile):
    """the fourth and fifth taxon are identical to one of the start tree: after the first insertion the new node is the only one
    whose subtree costs nothing, and the fifth taxon has one branch to go to, not three"""
    c = gc.early_cluster_case(8)
    e, got = _run(c, 1, tile)
    _kernel_built_it(e)
    assert e.Wp == 32 and gc.tiles_of(e.Wp, tile) == {0: 1, 1: 2, 2: 1, 4: 1, 8: 1}[tile]
    assert got == _host(c) == _oracle(c)
    _closed_form(c, got)


# ---- D. row tails
def _tail(c, tile, Wp, tiles, rows=4):
    e, got = _run(c, 1, tile)
    _kernel_built_it(e)
    assert e.S == rows and e.Wp == Wp and gc.tiles_of(e.Wp, tile, c.datatype) == tiles and e.num_informative == c.nsites
    assert got == _host(c) == _oracle(c)
    _closed_form(c, got)


@pytest.mark.parametrize("rem", gc.REMS)
@pytest.mark.parametrize("tile,Wp,tiles", gc.TAIL_DNA)
def test_row_tails_dna(tile, Wp, tiles, rem):
    """24 taxa; three splits have their columns in the last live word only (rem sites of it are alignment, 0 = all 32), four have
    none.  Lanes past the row end (64- and 128-word tiles at Wp 32, 96, 160) load the row's last words -- these words -- once
    more and must count nothing."""
    _tail(gc.tail_case(Wp, rem), tile, Wp, tiles)


@pytest.mark.parametrize("rem", gc.REMS)
@pytest.mark.parametrize("datatype,Wp,tiles", gc.TAIL_OTHER)
def test_row_tails_protein_and_32_state(datatype, Wp, tiles, rem):
    """five and eight rows per quad, 16-word tiles"""
    _tail(gc.tail_case(Wp, rem, datatype), None, Wp, tiles, rows={gc.AA: 20, gc.GENERIC: 32}[datatype])


@pytest.mark.parametrize("tile,datatype", [(t, gc.DNA) for t in gc.DNA_TILES] + [(None, gc.AA), (None, gc.GENERIC)])
def test_row_tails_with_homoplasy(tile, datatype):
    """the same tree with 48 columns that fit no tree: what U a walked child starts from matters below it (a second child whose
    sibling is not walked takes it from the registers of the expansion before, not from the parked vectors)"""
    c = gc.noisy_case(datatype)
    e, got = _run(c, 1, tile)
    _kernel_built_it(e)
    assert e.Wp == 32 and gc.tiles_of(e.Wp, tile, datatype) == ({0: 1, 1: 2, 2: 1, 4: 1, 8: 1}[tile] if datatype == gc.DNA else 2)
    assert got == _host(c) == _oracle(c)
    assert got["score"] > c.closed[-1]
