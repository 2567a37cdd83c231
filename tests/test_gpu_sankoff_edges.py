"""Edge cases of the weighted (Sankoff) engine's core kernels -- k_snk_pack, k_snk_newview(_wg), k_snk_evaluate, k_snk_pattern,
k_snk_scan, k_snk_scan_deep -- against the plain int64 reference (oracle/sankoff_slow.py) and the oracle's Sankoff mode.

The inputs come from tests/sankoff_edge_cases.py; tests/test_oracle_sankoff.py checks on the CPU that oracle and plain reference agree
on every one of them.  Every number is an integer and is compared exactly.  Every engine asserts the path it ran on: the store
(`sankoff_packed`), the state rows (`kernel_states`), the row pitch (`Wp`), and in group E the addressing (`snk_scan_wide`).

Groups: A row, element and tile edges; B tiny trees; C deep and flat trees; D both sides of the 16-bit gate; E wide addresses in the
scan; F live re-weighting and the alignment without an informative pattern.
"""
import numpy as np
import pytest

import sankoff_edge_cases as sec
from helpers import trace_tokens

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from mpboot_amd import engine
    from oracle import pyoracle as po
    return engine, po


def _oracle(po, case, weights=None):
    return po.Oracle(case["codes"], case["weights"] if weights is None else weights, datatype=case["datatype"], cost=case["cost"])


def _scan_nodes(po, case):
    o = _oracle(po, case)
    o.reset_nodep()
    n = case["codes"].shape[0]
    return sec.spread(o.nodep()[1:2 * n - 1], case["nodes"])


_ORACLE = {}
THEN_VISITS = 60          # prune-node visits of a climb's continuation at a deep radius (option max_visits, the oracle has the same switch)


def oracle_answers(po, case, weights=None, climb_radius=6, back=None, then_radius=0):
    """what the oracle gives for a case, computed once and shared by the engines it is compared with: score and per-pattern lengths of
    the start tree, the traces of the scanned prune nodes per radius, one climb and one randomized stepwise addition + SPR"""
    key = (case["name"], None if weights is None else np.asarray(weights).tobytes(), climb_radius, None if back is None else back.tobytes(),
           then_radius)
    if key in _ORACLE:
        return _ORACLE[key]
    back = case["back"] if back is None else back
    o = _oracle(po, case, weights)
    a = {"score": o.score_tree(back), "ninf": o.num_informative, "inf": o.informative().astype(bool)}
    a["ptn"], a["total"] = o.pattern_scores()
    o.reset_nodep()
    o.set_tree(back)
    o.score_tree()
    o.seed_ties(po.TIE_RANDOM, 1)
    a["nodes"] = _scan_nodes(po, case)
    a["scans"] = {}
    for radius in case["radii"]:
        for rec in a["nodes"]:
            o.set_best(a["score"])
            o.trace(True)
            o.rearrange(rec, 1, radius)
            a["scans"][radius, rec] = trace_tokens(*o.get_trace())
    if case.get("climb", True):
        o.set_tree(case.get("climb_back", back))
        o.seed_ties(po.TIE_RANDOM, 9)
        o.trace(True)
        s = o.optimize_spr(1, climb_radius)
        a["climb"] = (s, [x.tolist() for x in o.get_moves()], o.get_tree().tolist(), o.tie_state())
        if then_radius:                                # the climb goes on from where it ended, at a longer radius, for THEN_VISITS prune nodes
            done = len(a["climb"][1][0])                # (the oracle's move list goes on, the engine's starts again with each climb)
            o.set_max_visits(THEN_VISITS)
            s = o.optimize_spr(1, then_radius)
            o.set_max_visits(0)
            a["then"] = (s, [x.tolist()[done:] for x in o.get_moves()], o.get_tree().tolist(), o.tie_state())
    if case.get("ras", True):
        o.seed_ties(po.TIE_RANDOM, 4)
        s = o.make_tree(42, 3)[0]
        a["ras"] = (s, o.get_tree().tolist(), o.tie_state())
    _ORACLE[key] = a
    return a


def make_engine(engine, case, short, weights=None, force_big=None, kwords=0):
    """an engine in the 16-bit (short = 1) or the 32-bit store, with the path assertions every case makes"""
    n = case["codes"].shape[0]
    e = engine.FitchEngine(case["codes"], case["weights"] if weights is None else weights, datatype=case["datatype"], cost=case["cost"])
    if force_big is not None:
        e.set_option("force_big", force_big)
    if kwords:
        e.set_option("deep_scratch_kwords", kwords)
    e.set_option("sankoff_short", short)
    fits, _highest = sec.expect_packed(case["cost"], case["datatype"], n)
    assert e.get_option("sankoff_packed") == (1 if short and fits else 0)
    assert e.get_option("kernel_states") == sec.kernel_states(case["datatype"])
    return e


def check_geometry(e, ninf):
    assert e.num_informative == ninf
    assert e.Wp == max(32, 32 * ((ninf + 31) // 32))


def scan_tokens(e, rec, radius):
    q, mp, n_p = e.spr_scan(int(rec), 1, radius)
    return ["P"] + [f"{a}:{b}" for a, b in zip(q[:n_p], mp[:n_p])] + ["Q"] + [f"{a}:{b}" for a, b in zip(q[n_p:], mp[n_p:])], q, mp, n_p


def engine_answers(engine, e, case, want, weights=None, climb_radius=6, back=None, slow=True, then_radius=0):
    """the same calls on the engine, each compared with the oracle's answer (`want`) and, where `slow`, with the plain reference:
    score, per-pattern lengths, every candidate of the scanned prune nodes (none skipped: the token lists are equal in length and
    order), the climb and the stepwise addition.  -> everything it saw, for engine-against-engine comparisons; "deep_scans" counts
    the scans that launch_scan gave to k_snk_scan_deep (read-only option snk_scan_deep)"""
    back = case["back"] if back is None else back
    seen = {}
    s = e.score_tree(back)
    ptn, total = e.pattern_scores()
    assert s == want["score"] == total == want["total"]
    assert (ptn == want["ptn"]).all()
    if slow:
        ref, rptn = sec.slow_tree(case, back, weights)
        assert s == ref and (ptn[want["inf"]] == rptn[want["inf"]]).all() and not ptn[~want["inf"]].any()
    seen["score"], seen["ptn"] = s, ptn.tolist()
    tests = 0
    seen["deep_scans"] = 0
    for (radius, rec), toks in want["scans"].items():
        e.set_tree(back)
        mine, q, mp, n_p = scan_tokens(e, rec, radius)
        assert mine == toks, (case["name"], radius, rec)
        if len(q):
            seen["deep_scans"] += e.get_option("snk_scan_deep")
        seen["scan", radius, rec] = mine
        if slow:
            for k, (a, m) in enumerate(zip(q, mp)):
                prune = rec if k < n_p else int(back[rec])
                assert sec.slow_candidate(case, prune, int(a), back, weights) == int(m), (case["name"], radius, rec, int(a))
        tests += len(q)
    seen["tests"] = tests
    if "climb" in want:
        e.set_tree(case.get("climb_back", back))
        e.seed_ties(engine.TIE_RANDOM, 9)
        s = e.optimize_spr(1, climb_radius)
        seen["climb"] = (s, [x.tolist() for x in e.moves()], e.get_tree().tolist(), e.tie_state())
        assert seen["climb"] == want["climb"]
    if "then" in want:
        e.set_option("max_visits", THEN_VISITS)
        s = e.optimize_spr(1, then_radius)
        e.set_option("max_visits", 0)
        seen["then"] = (s, [x.tolist() for x in e.moves()], e.get_tree().tolist(), e.tie_state())
        assert seen["then"] == want["then"]
    if "ras" in want:
        e.seed_ties(engine.TIE_RANDOM, 4)
        s = e.make_parsimony_tree(42, 3)
        seen["ras"] = (s, e.get_tree().tolist(), e.tie_state())
        assert seen["ras"] == want["ras"]
    return seen


def both_stores(engine, po, case, kwords=None, climb_radius=6, then_radius=0, after=None):
    """kwords(short) -> deep_scratch_kwords of that store's engine; after(e, seen, short): further assertions on each engine"""
    want = oracle_answers(po, case, climb_radius=climb_radius, then_radius=then_radius)
    seen = []
    for short in (1, 0):
        e = make_engine(engine, case, short, kwords=kwords(short) if kwords else 0)
        if case["ninf"] is not None:
            check_geometry(e, case["ninf"])
        seen.append(engine_answers(engine, e, case, want, climb_radius=climb_radius, then_radius=then_radius))
        if after:
            after(e, seen[-1], short)
    assert seen[0] == seen[1]
    return seen[0]


# ---- A: row, element and tile edges
@pytest.mark.parametrize("kind,ninf", sec.A_PARAMS)
def test_row_element_and_tile_edges(mods, kind, ninf):
    """9 taxa, exactly ninf informative patterns between dropped columns (the kept patterns' indices are not 0, 1, 2, ...): rows of
    We = Wp elements (32-bit store) or Wp / 2 (16-bit store: a multiple of 16, the last 64-lane tile partly valid; an odd ninf leaves
    a padded upper half in the last pair), weights 0, 1, 7, 65 535 and 100 000 on the first pattern, the last one and its pair
    partner.  Every prune node at radius 3, a climb and a stepwise addition."""
    engine, po = mods
    case = sec.case_a(kind, ninf)
    assert case["codes"].shape[1] > ninf and sec.HEAVY[ninf % 5] in case["weights"].tolist()
    seen = both_stores(engine, po, case)
    assert seen["tests"] > 0


# ---- B: tiny trees
@pytest.mark.parametrize("n,kind", sec.B_PARAMS)
def test_tiny_trees(mods, n, kind):
    """4, 5 and 6 taxa (the radius is clipped to ntips - 3: 1, 2 and 3): the score of EVERY topology, every scan at radii 1 and 6, a
    climb, a stepwise addition"""
    engine, po = mods
    case = sec.case_b(n, kind)
    seen = both_stores(engine, po, case)
    assert seen["tests"] > 0
    o = _oracle(po, case)
    for short in (1, 0):
        e = make_engine(engine, case, short)
        for b in case["every_tree"]:
            s = e.score_tree(b)
            ptn, total = e.pattern_scores()
            ref, rptn = sec.slow_tree(case, b)
            assert s == total == ref == o.score_tree(b)
            assert (ptn == o.pattern_scores()[0]).all()


# ---- C: deep and flat trees
@pytest.mark.parametrize("which", sec.C_PARAMS)
def test_deep_and_flat_trees(mods, which):
    """a caterpillar of 128 taxa (DNA) and of 64 (protein): dependency levels near n in k_snk_newview_wg, scan chains as long as the
    radius allows -- radius 6 in registers, radius 13 in k_snk_scan_deep, whose scratch is sized for ONE wave-set of 14 levels, so
    that every batch of two and more scans is cut into several launches: 12 spread prune nodes at both radii, a climb at radius 6
    and its continuation at radius 13 (DNA) or 8 (protein: the deep kernel above 6 levels), whole sweeps of deep scans in batches.  What was dispatched is asserted: the radius-13 scans
    ran in the deep kernel, and the deep batches took more launches than there were batches.
    The balanced tree of 64 taxa under a matrix that is not symmetric is the flat end: its longest chains have 9 to 10 levels, so it
    stays in the DNA register kernel (12 levels) at its deepest instantiation at any radius, and nothing deep is asserted there."""
    engine, po = mods
    case = sec.case_c(which)
    S = sec.kernel_states(case["datatype"])

    def kwords(short):                                   # 14 levels x S rows x 64 lanes per wave, a wave per tile of 64 elements
        we = case["ninf"] + (-case["ninf"]) % 32
        tiles = ((we // 2 if short else we) + 63) // 64
        return (14 * S * 64 * tiles + 1023) // 1024

    def after(e, seen, short):
        if which.startswith("caterpillar"):
            assert seen["deep_scans"] > 0
            assert e.get_option("snk_deep_launches") > e.get_option("snk_deep_batches") > seen["deep_scans"]
        else:
            assert seen["deep_scans"] == 0

    seen = both_stores(engine, po, case, kwords=kwords, then_radius=13 if case["datatype"] == sec.DNA else 8, after=after)
    assert seen["tests"] > 100


# ---- D: both sides of the 16-bit gate
@pytest.mark.parametrize("gate,matrix", sec.D_PARAMS)
def test_both_sides_of_the_16_bit_gate(mods, gate, matrix):
    """The store is packed while 3 n highest_cost < 2^16, highest_cost = largest entry of the closed matrix + 1 (binary data in the
    4-row kernels: the added rows are filled with largest + 1 first, which moves the gate by one).  aa20: 3 x 20 x 1092 = 65 520
    packed, 3 x 20 x 1093 = 65 580 not; dna9: 3 x 9 x 2427 = 65 529 packed, 3 x 9 x 2428 = 65 556 not; bin9: the caller's largest
    entry 2425 gives highest_cost 2427, packed, 2426 gives 2428, not.  Matrices: the scaled unit matrix, a metric that is its own
    closure.  12 columns in which the taxa differ as far as the alphabet allows, then random ones.

    What the packed side stores (tests/test_oracle_sankoff.py::test_largest_stored_value_inside_the_16_bit_gate asserts it on the
    CPU, over the start tree and every rearrangement scanned here; n x highest_cost is 21 840 / 21 843 / 21 843):
        aa20  unit matrix: view entry 20 729, sum of three 20 729;  metric: 13 201 and 14 127
        dna9  unit matrix: view entry 16 982, sum of three 19 408;  metric: 12 186 and 14 045
        bin9  unit matrix: view entry 14 552, sum of three 16 978;  the other matrix: 14 540 and 16 972
    all below 65 536.  A view entry stays below n x highest_cost < 2^15, so the top bit of a 16-bit half is never reached inside the gate, and a sum of
    three transforms stays below 3 n highest_cost < 2^16.  Packed and unpacked engines must give identical numbers on both sides of
    the gate, equal to the plain reference's."""
    engine, po = mods
    for over in (0, 1):
        case = sec.case_d(gate, matrix, over)
        n = case["codes"].shape[0]
        fits, highest = sec.expect_packed(case["cost"], case["datatype"], n)
        assert fits == (over == 0)
        assert 3 * n * (highest + 1) >= 65536 if fits else 3 * n * (highest - 1) < 65536      # the two sides are neighbours
        e = make_engine(engine, case, 1)
        assert e.get_option("sankoff_packed") == 1 - over
        both_stores(engine, po, case)


# ---- E: wide addresses in the weighted scan
@pytest.mark.parametrize("name,kind", sec.E_PARAMS)
def test_wide_addresses_in_the_weighted_scan(mods, name, kind):
    """force_big on a weighted engine: k_snk_scan / k_snk_scan_deep <..., BUF = false> (64-bit pointers per row, what a half of the
    store of 4 GiB and more takes) -- DNA, protein and 32 states, both stores, symmetric and not, radii 6 and 13.  `snk_scan_wide`
    and `snk_scan_deep` tell what launch_scan dispatched: wide exactly under force_big; deep on morph32_40, dna_48 and the protein
    caterpillar, whose radius-13 scans go below the levels the registers keep, and never on dna_ambig and aa, whose trees are too
    small for that (sec.E_DEEP).  All four engines give the oracle's numbers (this group is compared with the oracle alone)."""
    engine, po = mods
    case = sec.case_e(name, kind)
    want = oracle_answers(po, case)
    seen = []
    for big in (0, 1):
        for short in (1, 0):
            e = make_engine(engine, case, short, force_big=big)
            assert e.get_option("snk_scan_wide") == 0 and e.get_option("snk_scan_deep") == 0        # no scan yet
            seen.append(engine_answers(engine, e, case, want, slow=False))
            assert e.get_option("snk_scan_wide") == big
            assert (seen[-1]["deep_scans"] > 0) == case["deep"] == (e.get_option("snk_deep_batches") > 0)
    assert all(s == seen[0] for s in seen[1:]) and seen[0]["tests"] > 0


@pytest.mark.parametrize("name,radius", [("dna_ambig", 6), ("aa", 8), ("dna_48", 13)])
def test_wide_addresses_under_the_tracker(mods, name, radius):
    """a tracked climb (-bb): the scan writes every tentative tree's per-pattern lengths (vals) and their maximum (vmax) through
    the wide variant -- of the register kernel on dna_ambig and aa, of the deep kernel as well on dna_48 at radius 13 (asserted)"""
    engine, po = mods
    case = sec.case_e(name, "sym")
    start = case.get("climb_back", case["back"])
    P = case["codes"].shape[1]
    w = case["weights"].astype(np.float64)
    samples = np.random.default_rng(4).multinomial(int(w.sum()), w / w.sum(), size=11).astype(np.uint16)
    o = _oracle(po, case)
    o.seed_ties(po.TIE_RANDOM, 5)
    o.ufboot_attach(samples)
    o.set_tree(start)
    o.trace(True)
    want = (o.optimize_spr(1, radius), [a.tolist() for a in o.get_moves()], o.get_tree().tolist(), o.ufboot_tree_logl().tolist(),
            [x.tolist() for x in o.ufboot_state()])
    assert len(samples[0]) == P
    for big in (0, 1):
        for short in (1, 0):
            e = make_engine(engine, case, short, force_big=big)
            e.seed_ties(engine.TIE_RANDOM, 5)
            e.ufboot_attach(samples)
            e.set_tree(start)
            got = (e.optimize_spr(1, radius), [a.tolist() for a in e.moves()], e.get_tree().tolist(), e.ufboot_tree_logl().tolist(),
                   [x.tolist() for x in e.ufboot_state()])
            assert got == want
            assert e.get_option("snk_scan_wide") == big
            if name != "aa":                 # (11 taxa at radius 8: a climb may or may not go below 6 levels; nothing is claimed)
                assert (e.get_option("snk_deep_batches") > 0) == (name == "dna_48")


# ---- F: live re-weighting, and the alignment without an informative pattern
@pytest.mark.parametrize("kind", sec.F_PARAMS)
def test_live_reweighting(mods, kind):
    """one engine through ones -> zeros and heavy weights -> ones: the row pitch stays, the pattern weights go up again each time;
    score, per-pattern lengths, a scan, a climb and a stepwise addition == the oracle's, the plain reference's and a fresh engine's"""
    engine, po = mods
    case = sec.case_f(kind)
    for short in (1, 0):
        e = make_engine(engine, case, short)
        check_geometry(e, case["ninf"])
        wp = e.Wp
        for w in case["weight_vectors"]:
            want = oracle_answers(po, case, weights=w)
            e.set_weights(w)
            assert e.Wp == wp and e.get_option("sankoff_packed") == short
            live = engine_answers(engine, e, case, want, weights=w)
            fresh = engine_answers(engine, make_engine(engine, case, short, weights=w), case, want, weights=w)
            assert live == fresh and live["tests"] > 0


def test_no_informative_pattern_under_a_cost_matrix(mods):
    """ninf = 0: one row of 32 padded patterns, every length 0 (the calls of test_gpu_edges.py::test_all_patterns_uninformative and
    the rest of this file's)"""
    engine, po = mods
    case = sec.case_f_empty()
    for short in (1, 0):
        e = make_engine(engine, case, short)
        check_geometry(e, 0)
        assert e.score_tree(case["back"]) == 0
        e.seed_ties(engine.TIE_RANDOM, 1)
        assert e.optimize_spr(1, 6) == 0
    seen = both_stores(engine, po, case)
    assert seen["score"] == 0 and not any(seen["ptn"])
