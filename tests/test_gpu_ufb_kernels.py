"""The UFBoot kernels of mpboot_amd/csrc/ufboot.hip, each against a plain exact reference (tests/ufb_probe.py), at the shapes where
its launcher takes another path.  Every product case asserts what launch_bitgemm dispatched (BitgemmRan) and the whole of C, the
padding rows excluded; every event size goes through every extraction route it can take.  Integer throughout: tolerance zero."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ufb_probe as up

pytestmark = pytest.mark.gpu

SPECIAL_SITES = (0, 15, 16, 31, 32, 47, 63, 64)


# ------------------------------------------------------------------------------------------------ inputs of the product
def make_masks(rows, Wp, rng):
    """Random rows; from 16 rows on also all ones, all zero and single bits at the sites where a fragment, a word or a k-block ends."""
    m = rng.integers(0, 2 ** 32, (rows, Wp), dtype=np.uint64).astype(np.uint32)
    if rows >= 16:
        m[1], m[2] = 0xFFFFFFFF, 0
        for k, site in enumerate(SPECIAL_SITES + (32 * Wp - 1,)):
            m[3 + k] = 0
            m[3 + k, site >> 5] = np.uint32(1) << np.uint32(site & 31)
        m[rows - 1] = 0xFFFFFFFF                       # (the last row of the product, next to the padding)
    return m


def make_weights(Wp, n_cols, rng):
    """Bytes 0..127, distinct per (site, column) inside every k-block, with 0, 1 and 127 present; every site carries a pattern."""
    P = 32 * Wp
    src = up.distinct_weights(P, n_cols, rng)
    src[rng.random(src.shape) < 0.05] = 0
    src[0, :3] = (0, 1, 127)
    return src, np.arange(P, dtype=np.int32), np.ones(P, np.int32)


def run_product(rows, Wp, Bp, want_ran, chained=True, seed=0, n_cols=None):
    rng = np.random.default_rng(seed + rows + 7 * Wp + Bp)
    n_cols = Bp - 3 if n_cols is None else n_cols
    masks = make_masks(rows, Wp, rng)
    src, first, cur = make_weights(Wp, n_cols, rng)
    noise = rng.integers(-2 ** 31, 2 ** 31 - 1, (up.padded_rows(rows, Bp, chained), Bp)).astype(np.int32)
    got, ran = up.product(masks, src, first, cur, Bp, chained=chained, prefill=noise)        # accumulate = 0: the noise must go
    assert ran == [want_ran], ran
    want = up.ref_product(masks, src.T)
    if rows * Wp <= 4096:
        assert (up.ref_product_int(masks, src.T) == want).all()
    assert (got[:rows, :n_cols] == want).all(), np.argwhere(got[:rows, :n_cols] != want)[:8]
    assert (got[:rows, n_cols:] == 0).all()
    return got


def ran(tm, tn, ksplit, per, gx, atomic, m32=0):
    return dict(tm=tm, tn=tn, ksplit=ksplit, kb_per_split=per, grid_x=gx, atomic=atomic, m32=m32)


# ------------------------------------------------------------------------------------------------ product: the tile shapes
@pytest.mark.parametrize("rows,Wp,Bp,want", [
    (1, 32, 256, ran(128, 128, 1, 16, 8, 0)),          # no split, plain stores, XCD map with idle workgroups (8 for 2 tiles)
    (129, 64, 256, ran(128, 128, 2, 16, 8, 1)),        # two K-splits: atomics behind the memset
    (2048, 160, 768, ran(128, 128, 3, 28, 96, 1)),     # six column blocks (generic map), splits of 28 / 28 / 24 k-blocks
    (801, 224, 1024, ran(128, 128, 5, 24, 56, 1)),     # nkb 112: four splits of 24 and a last one of 16
    (2048, 32, 256, ran(128, 128, 1, 16, 32, 0)),      # the last row count on 128-row tiles ...
], ids=["1x32x256", "129x64x256", "2048x160x768", "801x224x1024", "2048x32x256"])
def test_product_128_tile(rows, Wp, Bp, want):
    assert up.padded_rows(rows, Bp, True) == (rows + 127) // 128 * 128
    run_product(rows, Wp, Bp, want)


@pytest.mark.parametrize("rows,Wp,Bp,want", [
    (2049, 32, 256, ran(256, 256, 1, 16, 16, 0)),      # ... and the first on 256 x 256 (2560 padded rows, ten row blocks on 16 workgroups)
    (2049, 64, 256, ran(256, 256, 2, 16, 16, 1)),
    (2049, 64, 768, ran(256, 256, 2, 16, 30, 1)),      # three column blocks: the generic map
], ids=["2049x32x256", "2049x64x256", "2049x64x768"])
def test_product_256_tile(rows, Wp, Bp, want):
    assert up.padded_rows(rows, Bp, True) == 2560 == up.padded_rows(rows, Bp, False)
    run_product(rows, Wp, Bp, want)


@pytest.mark.parametrize("Bp,gx_per_rb", [(128, None), (384, 3)])
@pytest.mark.parametrize("rows,Wp", [(1, 32), (512, 32), (513, 32), (513, 64)])
def test_product_512_tile(rows, Wp, Bp, gx_per_rb):
    rb = (rows + 511) // 512
    assert up.padded_rows(rows, Bp, True) == 512 * rb
    ks = Wp // 32
    gx = 8 if gx_per_rb is None else gx_per_rb * rb    # one column block: the XCD map's eight; three: the generic map
    run_product(rows, Wp, Bp, ran(512, 128, ks, 16, gx, int(ks > 1)))


@pytest.mark.parametrize("Bp,tm,gx", [(128, 512, 8), (256, 128, 8)])
@pytest.mark.parametrize("Wp", [8, 16, 24])
def test_product_short_k(Wp, Bp, tm, gx):
    """nkb 4, 8, 12 (the weighted tracker's widths, rows padded to 512): at most three stages, the prefetch clamps onto them."""
    per = (Wp // 2 + 3) // 4 * 4
    run_product(37, Wp, Bp, ran(tm, 128, 1, per, gx, 0), chained=False)


# ------------------------------------------------------------------------------------------------ product: the options
@pytest.fixture(scope="module")
def acc_case():
    rng = np.random.default_rng(11)
    rows, Wp, Bp, n_cols = 300, 64, 256, 250
    masks = make_masks(rows, Wp, rng)
    src, first, cur = make_weights(Wp, n_cols, rng)
    pre = rng.integers(-10 ** 6, 10 ** 6, (up.padded_rows(rows, Bp, True), Bp)).astype(np.int32)
    return dict(rows=rows, Wp=Wp, Bp=Bp, n_cols=n_cols, masks=masks, src=src, first=first, cur=cur, pre=pre, ref=up.ref_product(masks, src.T))


@pytest.mark.parametrize("mult", [1, 128, 16384, 3 << 7])
def test_product_accumulates_with_mult(acc_case, mult):
    c = acc_case
    got, r = up.product(c["masks"], c["src"], c["first"], c["cur"], c["Bp"], mult=mult, accumulate=1, prefill=c["pre"])
    assert r == [ran(128, 128, 2, 16, 8, 1)]           # (three row blocks x two column blocks: eight workgroups on the XCD map)
    want = c["pre"][:c["rows"]].astype(np.int64)
    want[:, :c["n_cols"]] += mult * c["ref"]
    assert np.abs(want).max() < 2 ** 31
    assert (got[:c["rows"]] == want).all()


@pytest.mark.parametrize("kind", ["repeats", "permutation"])
def test_product_rowsel(acc_case, kind):
    c = acc_case
    rng = np.random.default_rng(5)
    rows, rp = (200, 256) if kind == "repeats" else (c["rows"], 384)
    sel = np.zeros(rp, np.uint32)
    sel[:rows] = rng.integers(0, 40, rows) if kind == "repeats" else rng.permutation(rows)
    assert kind != "repeats" or len(set(sel[:rows].tolist())) < rows
    got, r = up.product(c["masks"], c["src"], c["first"], c["cur"], c["Bp"], rows=rows, rowsel=sel)
    assert r == [ran(128, 128, 2, 16, 8 * ((rp // 128 + 3) // 4), 1)]
    assert (got[:rows, :c["n_cols"]] == c["ref"][sel[:rows]]).all()
    assert (got[:rows, c["n_cols"]:] == 0).all()


@pytest.mark.parametrize("limit", [0, 128, 129, 384, 1000])
def test_product_row_limit(acc_case, limit):
    """Row blocks that start at or behind the limit keep what C held, bit for bit; those in front hold the sum."""
    c = acc_case
    got, r = up.product(c["masks"], c["src"], c["first"], c["cur"], c["Bp"], accumulate=1, prefill=c["pre"], row_limit=limit)
    assert r == [ran(128, 128, 2, 16, 8, 1)]
    want = c["pre"].astype(np.int64)
    live = min(384, (limit + 127) // 128 * 128)
    hi = min(live, c["rows"])
    want[:hi, :c["n_cols"]] += c["ref"][:hi]
    assert (got[:hi] == want[:hi]).all()
    assert live in (0, 128, 256, 384) and (got[live:] == c["pre"][live:]).all()


@pytest.mark.parametrize("planes,top", [(1, 127), (2, 16383), (3, 65535)])
def test_product_weight_planes(planes, top):
    """launch_ufb_layout + one product per 7-bit plane against the sum over patterns (no fragment order restated)."""
    rng = np.random.default_rng(planes)
    rows, Wp, Bp, P, n_cols = 150, 64, 256, 333, 21
    masks = make_masks(rows, Wp, rng)
    sites = [0, 31, 32, 63, 64, 127, 32 * Wp - 64, 32 * Wp - 1]       # both ends of word pairs, the first and the last k-block
    rest = [s for s in rng.permutation(32 * Wp).tolist() if s not in sites]
    first = np.array(sites + rest[:P - len(sites)], np.int32)
    src = rng.integers(0, top + 1, (n_cols, P)).astype(np.uint16)
    edge = [w for w in (127, 128, 16383, 16384, 65535) if w <= top]
    for k, w in enumerate(edge):
        src[:, k] = w                                    # on the special sites, in every column
        src[k, 20:40] = w
    src[:, 8] = 0
    cur = np.ones(P, np.int32)
    first[9], cur[10], cur[11] = -1, 0, -3
    got, r = up.product(masks, src, first, cur, Bp, planes=planes)
    assert r == [ran(128, 128, 2, 16, 8, 1)] * planes
    want = up.ref_chain(masks, src, first, cur)
    assert want.max() < 2 ** 31 and (want[1] == src.astype(np.int64)[:, (first >= 0) & (cur > 0)].sum(axis=1)).all()
    assert (got[:rows, :n_cols] == want).all()
    assert (got[:rows, n_cols:] == 0).all()


# ------------------------------------------------------------------------------------------------ bit planes
NPATS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@pytest.mark.parametrize("K", [1, 9, 16])
def test_vals_planes(K):
    rng = np.random.default_rng(K)
    for npat in NPATS:
        for rows in (1, 5):
            vals = rng.integers(0, 1 << K, (rows, npat)).astype(np.uint16)
            vals[rows - 1, npat - 1] |= 1 << (K - 1)
            vals[0, 0] |= 1 << (K - 1)
            Wp = (2 * ((npat + 63) // 64) + 7) // 8 * 8 + 8          # words behind the last pattern's tile, a row behind the last
            fill = rng.integers(1, 2 ** 32, (K, rows + 1, Wp), dtype=np.uint64).astype(np.uint32)
            got, _, _ = up.vals_planes(vals, K, fill)
            assert (got == up.ref_planes(vals, K, fill)).all(), (npat, rows)
            assert (got[:, :, 2 * ((npat + 63) // 64):] == fill[:, :, 2 * ((npat + 63) // 64):]).all() and (got[:, rows] == fill[:, rows]).all()


@pytest.mark.parametrize("K", [1, 9, 16])
@pytest.mark.parametrize("npat,Bp,tm", [(1, 128, 512), (65, 256, 128), (257, 128, 512), (257, 256, 128)])
def test_weighted_chain(npat, K, Bp, tm):
    """launch_vals_planes, then K x planes products with mult (1 << k) << 7 pl: vals x W."""
    rng = np.random.default_rng(npat + K)
    rows, n_cols = 5, Bp - 5
    vals = rng.integers(0, 1 << K, (rows, npat)).astype(np.uint16)
    vals[0, npat - 1] |= 1 << (K - 1)
    top = min(300, (2 ** 31 - 1) // (((1 << K) - 1) * npat))          # every sum fits C's 32 bits
    W = rng.integers(0, top + 1, (n_cols, npat)).astype(np.uint16)
    W[0, 0] = top
    Wp = (2 * ((npat + 63) // 64) + 7) // 8 * 8
    noise = rng.integers(-2 ** 31, 2 ** 31 - 1, (512, Bp)).astype(np.int32)
    planes, got, r = up.vals_planes(vals, K, np.zeros((K, 512, Wp), np.uint32), W=W, wplanes=2, Bp=Bp, c_fill=noise)
    per = (Wp // 2 + 3) // 4 * 4
    assert r == ran(tm, 128, 1, per, 8, 0)
    assert (planes == up.ref_planes(vals, K, np.zeros((K, 512, Wp), np.uint32))).all()
    assert (got[:rows, :n_cols] == up.ref_weighted(vals, W)).all()
    assert (got[rows:] == 0).all() and (got[:, n_cols:] == 0).all()      # zero planes behind the rows, zero weights behind the columns


# ------------------------------------------------------------------------------------------------ the small kernels
@pytest.mark.parametrize("Wp", [32, 96])
@pytest.mark.parametrize("S", [4, 20, 32])
def test_join_masks(S, Wp):
    rng = np.random.default_rng(S + Wp)
    nv, n_ops = 9, 7
    # sparse state sets, so that "no common state" is neither rare nor the rule
    vec = (rng.integers(0, 2 ** 32, (nv, S, Wp), dtype=np.uint64) & rng.integers(0, 2 ** 32, (nv, S, Wp), dtype=np.uint64)).astype(np.uint32)
    if S > 4:
        vec &= rng.integers(0, 2 ** 32, (nv, S, Wp), dtype=np.uint64).astype(np.uint32)
    ops = np.zeros((n_ops, 4), np.uint32)
    ops[:, 0], ops[:, 1] = rng.integers(0, nv, n_ops), rng.integers(0, nv, n_ops)
    ops[0, :2] = (nv - 1, nv - 1)
    want = up.ref_join_masks(vec, ops)
    assert 0 < int(up.unpack_bits(want).sum()) < want.size * 32
    assert (up.join_masks(vec, ops, S, Wp) == want).all()


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 200])
def test_colsum(rows):
    rng = np.random.default_rng(rows)
    for Bp in (128, 384):
        Cm = rng.integers(-10 ** 6, 10 ** 6, (rows, Bp)).astype(np.int32)
        Cm[:, 5] = 0
        noise = rng.integers(-2 ** 31, 2 ** 31 - 1, Bp).astype(np.int32)
        assert (up.colsum(Cm, noise) == Cm.astype(np.int64).sum(axis=0)).all()


def test_rt_update_and_column():
    rng = np.random.default_rng(2)
    for Bp, rows in ((128, 3), (384, 300)):
        Cm = rng.integers(-10 ** 6, 10 ** 6, (rows, Bp)).astype(np.int32)
        rt = rng.integers(-10 ** 6, 10 ** 6, Bp).astype(np.int32)
        for row, home in ((rows - 1, 0), (1, 1), (0, rows - 1)):
            assert (up.rt_update(rt, Cm, row, home) == rt.astype(np.int64) + Cm[row] - Cm[home]).all()
        for col, n in ((0, rows), (Bp - 1, rows), (77, rows - 1), (3, 0)):
            fill = rng.integers(-99, 99, rows + 2).astype(np.int32)
            want = fill.copy()
            want[:n] = Cm[:n, col]
            assert (up.column(Cm, col, n, fill) == want).all()


# ------------------------------------------------------------------------------------------------ events
N_IDX = (1, 15, 16, 17, 255, 256, 257, 1024, 1025, 4095, 4096, 4097)
SAMPLES = ((1, 128), (63, 128), (64, 128), (65, 128), (129, 256))
RANGES = ([], [5], list(range(1000)))


def check_publication(out, ranges, ev_cap_host):
    assert int(out["h_flag"][1]) == 1 and int(out["h_flag"][0]) == out["count"] and out["done"] == 0
    for k in range(3):
        assert out["dst"][k].tolist() == (list(ranges[k]) if k < len(ranges) else [])
    n = min(out["count"], ev_cap_host)
    assert (out["h_ev"][:n] == out["ev"][:n]).all()


@pytest.mark.parametrize("n_idx", N_IDX)
def test_events_every_route(n_idx):
    """launch_ufb_events: one chunk (n_idx <= 256), fused (<= 1024), chunk minima + prefix (above), fixed bound;
    launch_ufb_events_publish: k_ufb_events2 <false> / <true> up to 4096, the chunked kernels + k_ufb_publish above."""
    assert up.lib().mpf_probe_events2_max() == 4096 and up.lib().mpf_probe_chunks(n_idx) == (n_idx + 255) // 256
    for B, Bp in SAMPLES:
        case = up.make_event_case(n_idx, B, Bp, seed=n_idx + B)
        for crow in (False, True):
            scores = up.ref_scores(case, crow)
            for fixed in (False, True):
                want, count = up.ref_events(case, B, fixed=fixed, crow=crow, scores=scores)
                for route in (0, 1):
                    out = up.events(case, route, B, fixed=fixed, crow=crow, ranges=RANGES, ev_cap=count + 40, h_ev_cap=40)
                    what = (n_idx, B, crow, fixed, route)
                    assert out["count"] == count, what
                    assert len(out["ev"]) == count and (up.sorted_events(out["ev"]) == want).all(), what
                    if route == 1:
                        check_publication(out, RANGES, 40)


@pytest.fixture(scope="module")
def ev_case():
    case = up.make_event_case(700, 129, 256, seed=77)
    # best above R_T for half of the samples: a start of the running minimum that is one batch old
    case["best"][:129:2] = case["rt"][:129:2].astype(np.uint32) + 2
    # ... and no current-tree slot (score R_T itself) in front of the first candidates, which would hide the difference
    front = case["info"][:40]
    front[front[:, 1] == up.SELF] = (0, up.SKIP)
    return case


@pytest.mark.parametrize("cut", [None, 0, 21, 272, 699, 700, 5000])
@pytest.mark.parametrize("fixed", [False, True])
def test_events2_clamp_and_cut(ev_case, fixed, cut):
    """clamp_rt starts at min(best, R_T) (not under a fixed bound); cut inside a slice (21), inside a pass (272), at 0, at and
    behind n_idx."""
    want, count = up.ref_events(ev_case, 129, fixed=fixed, clamp_rt=not fixed, cut=cut)
    plain, _ = up.ref_events(ev_case, 129, fixed=fixed, cut=cut)
    assert fixed or cut == 0 or want.tolist() != plain.tolist()       # (the clamp changes what is expected here)
    ranges = ([7] * 1003, [1, 2, 3, 4, 5, 6, 7], [])
    out = up.events(ev_case, 1, 129, fixed=fixed, clamp_rt=True, cut=cut, ranges=ranges, h_ev_cap=count + 1)
    assert out["count"] == count == len(out["ev"]) and (up.sorted_events(out["ev"]) == want).all()
    check_publication(out, ranges, count + 1)


@pytest.mark.parametrize("n_idx,route", [(200, 0), (700, 0), (2000, 0), (700, 1), (4097, 1)])
def test_events_cap_below_the_count(n_idx, route):
    case = up.make_event_case(n_idx, 65, 128, seed=n_idx)
    want, count = up.ref_events(case, 65)
    cap = count // 3
    assert cap > 10
    out = up.events(case, route, 65, ev_cap=cap, h_ev_cap=cap // 2, ranges=RANGES)
    assert out["count"] == count
    got = up.event_set(out["ev"])
    assert len(out["ev"]) == cap == len(got) and got <= up.event_set(want)
    if route == 1:
        check_publication(out, RANGES, cap // 2)


def _self_slots(case):
    return np.array([i for i in range(case["n_idx"]) if int(case["info"][i][1]) in (up.SELF, up.SKIP) and int(case["info"][i][0]) == 0
                     and i not in set(case["home"].tolist())], np.uint32)


@pytest.mark.parametrize("c_words", [0, 512, 20000])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("code", [up.SELF, up.SKIP])
def test_mid_prep_self(kind, c_words, code):
    case = up.make_event_case(300, 4, 128, seed=c_words + kind)
    rng = np.random.default_rng(kind)
    idx = _self_slots(case)
    assert len(idx) > 20
    info = case["info"].copy()
    part_of = {int(p): k for k, p in enumerate(case["plan_end"])}
    for i in idx:                                        # what an earlier batch left there: a candidate cheaper than any home
        info[i] = (int(i), next(k for e, k in sorted(part_of.items()) if e > i))
    cost = case["cost"].copy()
    cost[:case["plan_end"][0]] = cost[case["home"][0]]   # the first part: every candidate ties its home, none is better
    cost[idx] = 0
    Cm = rng.integers(1, 2 ** 31 - 1, 20480).astype(np.int32)
    ranges = (cost.tolist(), info.reshape(-1).tolist()[:333], [9])
    out = up.mid(kind, Cm, c_words, info, idx, code, cost=cost, home=case["home"], plan_end=case["plan_end"], ranges=ranges)
    want_info = info.copy()
    want_info[idx] = (0, code)
    assert (out["info"] == want_info).all()
    if kind == 2:
        assert (out["C"] == Cm).all() and out["ev_count"] == 99 and out["cut"] == 0x12345678
        return
    assert (out["C"][:c_words] == 0).all() and (out["C"][c_words:] == Cm[c_words:]).all() and out["ev_count"] == 0
    if kind == 1:
        assert out["cut"] == 0x12345678
        return
    want_cut = up.ref_cut(want_info, cost, case["home"], case["plan_end"], 300)
    assert int(case["plan_end"][0]) < want_cut < 300 and want_cut == min(int(e) for k, e in enumerate(case["plan_end"])
                                               if any(int(want_info[i][1]) == k and cost[i] < cost[case["home"][k]] for i in range(300)))
    assert out["cut"] == want_cut and int(out["h_flag"][2]) == want_cut
    assert int(out["h_flag"][1]) == 1 and int(out["h_flag"][0]) == 0 and out["done"] == 0
    assert [d.tolist() for d in out["dst"]] == [list(r) for r in ranges]


def test_mid_without_a_better_candidate():
    case = up.make_event_case(300, 4, 128, seed=4)
    cost = case["cost"].copy()
    cost[case["home"]] = 0                              # no candidate is cheaper than its part's home
    out = up.mid(0, np.ones(64, np.int32), 64, case["info"], _self_slots(case), up.SELF, cost=cost, home=case["home"],
                 plan_end=case["plan_end"])
    assert out["cut"] == 300 == int(out["h_flag"][2]) == up.ref_cut(out["info"], cost, case["home"], case["plan_end"], 300)


# ------------------------------------------------------------------------------------------------ the launcher's options
# setting -> [(rows, Wp, Bp, accumulate, BitgemmRan)]: what launch_bitgemm dispatches under it (rows pad to 512 unless MPF_GEMM_SMALL is 2)
def _variant_grid(m32):
    return [(2049, 32, 256, 0, ran(256, 256, 1, 16, 16, 0, m32)), (2100, 64, 768, 1, ran(256, 256, 2, 16, 30, 1, m32))]


VARIANTS = {
    "MPF_GEMM_VARIANT=1": _variant_grid(0), "MPF_GEMM_VARIANT=2": _variant_grid(0), "MPF_GEMM_VARIANT=3": _variant_grid(0),
    "MPF_GEMM_VARIANT=4": _variant_grid(1), "MPF_GEMM_VARIANT=5": _variant_grid(1),
    "MPF_GEMM_SMALL=1": [(1, 32, 256, 0, ran(512, 128, 1, 16, 8, 0)), (600, 64, 768, 1, ran(512, 128, 2, 16, 12, 1))],
    "MPF_GEMM_SMALL=3": [(1, 32, 256, 0, ran(256, 128, 1, 16, 8, 0)), (600, 64, 768, 1, ran(256, 128, 2, 16, 24, 1))],
    "MPF_GEMM_SMALL=4": [(1, 32, 256, 0, ran(128, 256, 1, 16, 8, 0)), (600, 64, 768, 1, ran(128, 256, 2, 16, 24, 1))],
    # the largest split the launcher allows (nkb / 16), on small matrices
    "MPF_GEMM_WANT=4096": [(1, 32, 256, 0, ran(128, 128, 1, 16, 8, 0)), (129, 160, 256, 1, ran(128, 128, 5, 16, 8, 1)),
                           (513, 64, 128, 0, ran(512, 128, 2, 16, 8, 1))],
}


def run_reduced_grid(setting):
    """In a child process that has `setting` in its environment: the product with the same assertions, dispatch included."""
    name, value = setting.split("=")
    assert os.environ.get(name) == value
    for rows, Wp, Bp, acc, want in VARIANTS[setting]:
        rng = np.random.default_rng(rows)
        n_cols = Bp - 3
        masks = make_masks(rows, Wp, rng)
        src, first, cur = make_weights(Wp, n_cols, rng)
        pre = rng.integers(-10 ** 6, 10 ** 6, (up.padded_rows(rows, Bp, True), Bp)).astype(np.int32)
        got, r = up.product(masks, src, first, cur, Bp, accumulate=acc, prefill=pre, mult=128 if acc else 1)
        assert r == [want], (setting, rows, r)
        ref = up.ref_product(masks, src.T)
        expect = np.zeros((rows, Bp), np.int64)
        if acc:
            expect += pre[:rows]
        expect[:, :n_cols] += (128 if acc else 1) * ref
        assert (got[:rows] == expect).all(), (setting, rows, Wp, Bp)
    print("reduced grid ok:", setting)


_abnormal = []       # the setting whose child ended abnormally: nothing more is started on the GPU behind it


@pytest.mark.parametrize("setting", list(VARIANTS))
def test_product_under_launcher_option(setting):
    if _abnormal:
        pytest.fail(f"not started: the child for {_abnormal[0]} ended abnormally")
    env = dict(os.environ)
    name, value = setting.split("=")
    env[name] = value
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import test_gpu_ufb_kernels as t; t.run_reduced_grid({setting!r})"
    try:
        p = subprocess.run([sys.executable, "-c", code], cwd=here, env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _abnormal.append(setting)
        pytest.fail(f"{setting}: the child did not end within its time limit")
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _abnormal.append(setting)
    assert p.returncode == 0 and "reduced grid ok: " + setting in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
