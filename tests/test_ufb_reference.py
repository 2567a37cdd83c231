"""CPU checks of the plain references in tests/ufb_probe.py (what tests/test_gpu_ufb_kernels.py holds the UFBoot kernels to)
against slower independent forms on small inputs: bit loops for the products and the planes, a pure-Python walk per sample for
the events, hand-made examples for the batch's end.  No GPU, no library."""
import numpy as np
import pytest

import ufb_probe as up


def _bit(masks, row, site):
    return (int(masks[row][site >> 5]) >> (site & 31)) & 1


def _slow_product(masks, Wsite):
    rows, sites, cols = len(masks), Wsite.shape[0], Wsite.shape[1]
    out = [[0] * cols for _ in range(rows)]
    for r in range(rows):
        for s in range(sites):
            if _bit(masks, r, s):
                for c in range(cols):
                    out[r][c] += int(Wsite[s][c])
    return np.array(out, np.int64).reshape(rows, cols)


@pytest.mark.parametrize("rows,Wp,cols,top", [(1, 2, 1, 127), (5, 4, 3, 127), (9, 3, 7, 65535)])
def test_product_forms_agree_with_a_bit_loop(rows, Wp, cols, top):
    rng = np.random.default_rng(rows * 100 + Wp)
    masks = rng.integers(0, 2 ** 32, (rows, Wp), dtype=np.uint64).astype(np.uint32)
    masks[0] = 0xFFFFFFFF
    W = rng.integers(0, top + 1, (32 * Wp, cols))
    want = _slow_product(masks, W)
    assert (up.ref_product(masks, W) == want).all()
    assert (up.ref_product_int(masks, W) == want).all()
    assert (want[0] == W.sum(axis=0)).all()


def test_unpack_bits_site_order():
    m = np.zeros((1, 3), np.uint32)
    for site in (0, 15, 16, 31, 32, 47, 63, 64, 95):
        m[:] = 0
        m[0, site >> 5] = np.uint32(1) << np.uint32(site & 31)
        bits = up.unpack_bits(m)
        assert bits.shape == (1, 96) and bits.sum() == 1 and bits[0, site] == 1


def test_chain_against_a_loop_over_patterns():
    rng = np.random.default_rng(3)
    rows, Wp, P, cols = 6, 4, 37, 5
    masks = rng.integers(0, 2 ** 32, (rows, Wp), dtype=np.uint64).astype(np.uint32)
    src = rng.integers(0, 65536, (cols, P)).astype(np.uint16)
    src[:, 3] = 0
    first = rng.permutation(32 * Wp)[:P].astype(np.int32)
    first[5] = -1
    cur = rng.integers(0, 3, P).astype(np.int32)
    want = np.zeros((rows, cols), np.int64)
    for r in range(rows):
        for c in range(cols):
            for p in range(P):
                if first[p] >= 0 and cur[p] > 0 and _bit(masks, r, int(first[p])):
                    want[r, c] += int(src[c, p])
    assert (up.ref_chain(masks, src, first, cur) == want).all()
    # the planes the device stores (7 bits each) recompose to the same weights
    W = up.site_weights(src, first, cur, 32 * Wp)
    assert (sum(((W >> (7 * pl)) & 0x7F) << (7 * pl) for pl in range(3)) == W).all()


@pytest.mark.parametrize("npat,K,rows", [(1, 1, 1), (63, 9, 2), (65, 16, 3), (129, 16, 2)])
def test_planes_against_a_bit_loop(npat, K, rows):
    rng = np.random.default_rng(npat + K)
    vals = rng.integers(0, 1 << K, (rows, npat)).astype(np.uint16)
    vals[0, npat - 1] |= 1 << (K - 1)
    Wp, rows_p = 2 * ((npat + 63) // 64) + 2, rows + 1
    fill = np.full((K, rows_p, Wp), 0xC3C3C3C3, np.uint32)
    got = up.ref_planes(vals, K, fill)
    want = fill.copy()
    want[:, :rows, :Wp - 2] = 0
    for k in range(K):
        for r in range(rows):
            for j in range(npat):
                if (int(vals[r, j]) >> k) & 1:
                    want[k, r, j >> 5] |= np.uint32(1 << (j & 31))
    assert (got == want).all()
    # ... and the planes give the values back: sum_k 2^k plane_k x W = vals x W
    W = rng.integers(0, 65536, (4, npat)).astype(np.uint16)
    Wsite = np.zeros((32 * Wp, 4), np.int64)
    Wsite[:npat] = W.T
    zero = up.ref_planes(vals, K, np.zeros((K, rows_p, Wp), np.uint32))
    total = sum(up.ref_product_int(zero[k], Wsite) << k for k in range(K))
    assert (total[:rows] == up.ref_weighted(vals, W)).all() and (total[rows:] == 0).all()


def _slow_events(case, B, fixed, crow, n, run0):
    """One sample at a time, scalar Python, the rule restated on its own."""
    out = []
    Cm = case["C_crow"] if crow else case["C_direct"]
    for b in range(B):
        run = run0[b]
        for i in range(n):
            part = int(case["info"][i][1])
            if part == 0xFFFFFFFF:
                continue
            if part == 0xFFFFFFFE:
                s = int(case["rt"][b])
            else:
                if not int(case["cost"][i]) < int(case["thr"][part]):
                    continue
                h = int(case["home"][part])
                ri, rh = (int(case["crow"][i]), int(case["crow"][h])) if crow else (int(case["info"][i][0]), h)
                s = int(case["rt"][b]) - int(Cm[rh][b]) + int(Cm[ri][b])
            s %= 1 << 32
            if s <= run:
                out.append((i, b, s))
                if not fixed:
                    run = s
    return out


@pytest.mark.parametrize("crow", [False, True])
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("n_idx,B", [(1, 1), (17, 3), (300, 5)])
def test_events_against_a_walk_per_sample(n_idx, B, fixed, crow):
    case = up.make_event_case(n_idx, B, B + 3, seed=n_idx)
    kinds = {int(x) for x in case["info"][:, 1]}
    if n_idx >= 300:
        assert up.SKIP in kinds and up.SELF in kinds and len(kinds) > 2
        c, t = case["cost"], case["thr"][np.minimum(case["info"][:, 1], len(case["thr"]) - 1)]
        assert (c == t).any() and (c > t).any() and (c < t).any()
    best = [int(x) for x in case["best"]]
    want = _slow_events(case, B, fixed, crow, n_idx, best)
    got, count = up.ref_events(case, B, fixed=fixed, crow=crow)
    assert count == len(want) == len(set(want)) == len(got) and got.tolist() == [list(e) for e in sorted(want)]
    assert (up.sorted_events(got[::-1]) == got).all()
    if n_idx >= 300:
        assert 0 < count < n_idx * B
        # clamp and cut: the start of the running minimum and the end of the walk
        clamped = [min(best[b], int(case["rt"][b]) % (1 << 32)) for b in range(B)]
        assert up.event_set(up.ref_events(case, B, fixed=fixed, crow=crow, clamp_rt=True, cut=123)[0]) == set(_slow_events(case, B, fixed, crow, 123, clamped))
        assert up.ref_events(case, B, fixed=fixed, crow=crow, cut=0)[1] == 0


def test_event_case_has_ties_and_both_forms_score_alike():
    case = up.make_event_case(257, 9, 16, seed=1)
    a, b = up.ref_scores(case, False), up.ref_scores(case, True)
    assert (a[:, :9] == b[:, :9]).all()
    ev, _ = up.ref_events(case, 9)
    by_sample = {}
    for i, s_, v in ev.tolist():
        by_sample.setdefault(s_, []).append(v)
    assert any(any(x == y for x, y in zip(v, v[1:])) for v in by_sample.values())     # an event that only ties the minimum


def test_cut_examples():
    S, H = up.SELF, up.SKIP
    #        idx: 0        1       2       3       4        5       6       7
    info = np.array([(0, S), (1, 0), (2, 0), (3, H), (0, S), (5, 1), (6, 1), (7, H)], np.uint32)
    home, plan_end = [3, 7], [4, 8]
    assert up.ref_cut(info, [9, 5, 5, 5, 9, 5, 5, 5], home, plan_end, 8) == 8          # ties are not better
    assert up.ref_cut(info, [0, 5, 5, 5, 0, 5, 4, 5], home, plan_end, 8) == 8 - 0      # second part: its end
    assert up.ref_cut(info, [0, 5, 4, 5, 0, 5, 4, 5], home, plan_end, 8) == 4          # the first part that has one
    assert up.ref_cut(info, [0, 5, 5, 5, 0, 5, 5, 5], home, plan_end, 8) == 8          # the current tree's slots never count


def test_join_masks_against_a_loop():
    rng = np.random.default_rng(8)
    S, Wp, nv = 4, 3, 5
    vec = rng.integers(0, 2 ** 32, (nv, S, Wp), dtype=np.uint64).astype(np.uint32)
    ops = np.array([(0, 1, 0, 0), (4, 2, 1, 0), (3, 3, 2, 0)], np.uint32)
    got = up.ref_join_masks(vec, ops)
    for o, (a, b, _x, _y) in enumerate(ops.tolist()):
        for w in range(Wp):
            for j in range(32):
                common = any((int(vec[a, k, w]) >> j) & (int(vec[b, k, w]) >> j) & 1 for k in range(S))
                assert (int(got[o, w]) >> j) & 1 == (0 if common else 1)
