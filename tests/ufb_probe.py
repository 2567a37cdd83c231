"""The test-only way into the UFBoot kernels (mpboot_amd/libmpfprobe.so: ufboot.o behind the mpf_probe_* functions of
csrc/ufb_probe.cpp) and plain numpy references of what they compute.  Everything is integer: the references are exact.

The references restate the operations, not the kernels: a product is "unpack the bits, multiply", the weight chain is a sum over
patterns (no fragment order), the events are a walk over the indices per sample.  tests/test_ufb_reference.py checks them on the
CPU against slower independent forms; tests/test_gpu_ufb_kernels.py compares the kernels with them."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.environ.get("MPF_PROBE_PATH") or os.path.join(ROOT, "mpboot_amd", "libmpfprobe.so")

SKIP, SELF = 0xFFFFFFFF, 0xFFFFFFFE          # info[i][1]: a home slot / the current tree's slot; anything else is a part
NONE = 0xFFFFFFFF                            # "no score" (uint32)
RAN_FIELDS = ("tm", "tn", "ksplit", "kb_per_split", "grid_x", "atomic", "m32")

u32p, i32p, u16p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint16)


class _Product(C.Structure):
    _fields_ = [("masks", u32p), ("mask_rows", C.c_int32), ("rows", C.c_int32), ("rows_padded", C.c_int32), ("chained", C.c_int32),
                ("Wp", C.c_int32), ("Bp", C.c_int32), ("src", u16p), ("n_cols", C.c_int32), ("P", C.c_int32), ("first", i32p),
                ("cur", i32p), ("planes", C.c_int32), ("C", i32p), ("mult", C.c_int32), ("accumulate", C.c_int32), ("rowsel", u32p),
                ("have_limit", C.c_int32), ("row_limit", C.c_uint32), ("ran", i32p)]


class _Events(C.Structure):
    _fields_ = [("route", C.c_int32), ("info", u32p), ("cost", u32p), ("thr", u32p), ("home", u32p), ("crow", u32p), ("C", i32p),
                ("rt", i32p), ("best", u32p), ("n_idx", C.c_uint32), ("n_parts", C.c_uint32), ("c_rows", C.c_uint32), ("Bp", C.c_int32),
                ("B", C.c_int32), ("fixed_bound", C.c_int32), ("clamp_rt", C.c_int32), ("have_cut", C.c_int32), ("cut", C.c_uint32),
                ("ev", u32p), ("ev_cap", C.c_uint32), ("ev_count", u32p), ("pub_src", u32p * 3), ("pub_dst", u32p * 3),
                ("pub_words", C.c_uint32 * 3), ("h_ev", u32p), ("h_ev_cap", C.c_uint32), ("h_flag", u32p), ("done", u32p)]


class _Mid(C.Structure):
    _fields_ = [("kind", C.c_int32), ("C", i32p), ("c_total", C.c_uint32), ("c_words", C.c_uint32), ("info", u32p), ("self_idx", u32p),
                ("n_self", C.c_uint32), ("code", C.c_uint32), ("ev_count", u32p), ("cost", u32p), ("home", u32p), ("plan_end", u32p),
                ("n_idx", C.c_uint32), ("n_parts", C.c_uint32), ("cut", u32p), ("pub_src", u32p * 3), ("pub_dst", u32p * 3),
                ("pub_words", C.c_uint32 * 3), ("h_flag", u32p), ("done", u32p)]


_lib = None


def lib():
    """libmpfprobe.so; a missing library is an error (it is built with libmpfitch.so)."""
    global _lib
    if _lib is None:
        if not os.path.exists(PROBE_PATH):
            raise RuntimeError(f"{PROBE_PATH} has not been built (make -C mpboot_amd/csrc)")
        _lib = C.CDLL(PROBE_PATH)
        for name in ("mpf_probe_row_tile", "mpf_probe_row_padding", "mpf_probe_events2_max", "mpf_probe_chunks", "mpf_probe_product",
                     "mpf_probe_vals", "mpf_probe_join_masks", "mpf_probe_colsum", "mpf_probe_rt_update", "mpf_probe_column",
                     "mpf_probe_events", "mpf_probe_mid"):
            getattr(_lib, name).restype = C.c_int
        _lib.mpf_probe_row_padding.argtypes = [C.c_int, C.c_int]
        _lib.mpf_probe_chunks.argtypes = [C.c_uint32]
        _lib.mpf_probe_product.argtypes = [C.POINTER(_Product)]
        _lib.mpf_probe_events.argtypes = [C.POINTER(_Events)]
        _lib.mpf_probe_mid.argtypes = [C.POINTER(_Mid)]
        _lib.mpf_probe_vals.argtypes = [u16p, C.c_uint32, C.c_uint32, C.c_int, u32p, C.c_uint32, C.c_uint32, u16p, C.c_int, C.c_int, C.c_int,
                                        i32p, i32p]
        _lib.mpf_probe_join_masks.argtypes = [u32p, C.c_uint32, u32p, C.c_int, C.c_int, C.c_int, u32p]
        _lib.mpf_probe_colsum.argtypes = [i32p, C.c_int, C.c_int, i32p]
        _lib.mpf_probe_rt_update.argtypes = [i32p, i32p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32]
        _lib.mpf_probe_column.argtypes = [i32p, C.c_uint32, C.c_int, C.c_int, i32p, C.c_uint32]
    return _lib


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else typ()


def _ok(code, what):
    if code != 0:
        raise RuntimeError(f"{what}: hipError_t {code}")


def row_tile():
    return lib().mpf_probe_row_tile()


def padded_rows(rows, Bp, chained):
    """Rows of the padded product as the callers reserve them: ufb_row_padding for a chained batch, the 512-row tile otherwise."""
    unit = lib().mpf_probe_row_padding(rows, Bp) if chained else row_tile()
    return (rows + unit - 1) // unit * unit


def ran_dicts(ran):
    return [dict(zip(RAN_FIELDS, (int(x) for x in r))) for r in ran]


# ------------------------------------------------------------------------------------------------ the kernels
def product(masks, src, first, cur, Bp, planes=1, chained=True, rows=None, mult=1, accumulate=0, prefill=None, rowsel=None,
            row_limit=None):
    """launch_ufb_layout + launch_bitgemm per weight plane.  masks [mask_rows][Wp] uint32; src [n_cols][P] uint16; rows = rows of
    the product (default: those of masks).  Returns (C [rows_padded][Bp] int32, [BitgemmRan per plane])."""
    masks = _arr(masks, np.uint32)
    src, first, cur = _arr(src, np.uint16), _arr(first, np.int32), _arr(cur, np.int32)
    rows = masks.shape[0] if rows is None else rows
    rp = padded_rows(rows, Bp, chained)
    Cm = np.zeros((rp, Bp), np.int32) if prefill is None else _arr(prefill, np.int32).copy()
    assert Cm.shape == (rp, Bp)
    sel = None if rowsel is None else _arr(rowsel, np.uint32)
    assert sel is None or sel.shape == (rp,)
    ran = np.zeros((planes, 7), np.int32)
    a = _Product(_ptr(masks, u32p), masks.shape[0], rows, rp, int(bool(chained)), masks.shape[1], Bp, _ptr(src, u16p), src.shape[0],
                 src.shape[1], _ptr(first, i32p), _ptr(cur, i32p), planes, _ptr(Cm, i32p), mult, accumulate, _ptr(sel, u32p),
                 int(row_limit is not None), 0 if row_limit is None else row_limit, _ptr(ran, i32p))
    _ok(lib().mpf_probe_product(C.byref(a)), "mpf_probe_product")
    return Cm, ran_dicts(ran)


def vals_planes(vals, K, planes_in, W=None, wplanes=1, Bp=128, c_fill=None):
    """launch_vals_planes into a copy of planes_in [K][rows_p][Wp]; with W [n_cols][npat] also the weighted chain into C.
    Returns (planes, C or None, BitgemmRan of the first product or None)."""
    vals = _arr(vals, np.uint16)
    planes = _arr(planes_in, np.uint32).copy()
    assert planes.ndim == 3 and planes.shape[0] == K
    rows, npat = vals.shape
    rows_p, Wp = planes.shape[1], planes.shape[2]
    Wm = None if W is None else _arr(W, np.uint16)
    Cm = None
    if Wm is not None:
        Cm = np.zeros((rows_p, Bp), np.int32) if c_fill is None else _arr(c_fill, np.int32).copy()
        assert Cm.shape == (rows_p, Bp)
    ran = np.zeros((1, 7), np.int32)
    _ok(lib().mpf_probe_vals(_ptr(vals, u16p), rows, npat, K, _ptr(planes, u32p), rows_p, Wp, _ptr(Wm, u16p), 0 if Wm is None else Wm.shape[0],
                             wplanes, Bp, _ptr(Cm, i32p), _ptr(ran, i32p)), "mpf_probe_vals")
    return planes, Cm, (ran_dicts(ran)[0] if Wm is not None else None)


def join_masks(vec, ops, S, Wp):
    vec, ops = _arr(vec, np.uint32), _arr(ops, np.uint32)
    out = np.full((ops.shape[0], Wp), 0x5A5A5A5A, np.uint32)
    _ok(lib().mpf_probe_join_masks(_ptr(vec, u32p), vec.shape[0], _ptr(ops, u32p), ops.shape[0], S, Wp, _ptr(out, u32p)), "mpf_probe_join_masks")
    return out


def colsum(Cm, rt_noise):
    Cm, rt = _arr(Cm, np.int32), _arr(rt_noise, np.int32).copy()
    _ok(lib().mpf_probe_colsum(_ptr(Cm, i32p), Cm.shape[0], Cm.shape[1], _ptr(rt, i32p)), "mpf_probe_colsum")
    return rt


def rt_update(rt, Cm, row, home):
    Cm, rt = _arr(Cm, np.int32), _arr(rt, np.int32).copy()
    _ok(lib().mpf_probe_rt_update(_ptr(rt, i32p), _ptr(Cm, i32p), Cm.shape[0], Cm.shape[1], row, home), "mpf_probe_rt_update")
    return rt


def column(Cm, col, rows, out_fill):
    Cm, out = _arr(Cm, np.int32), _arr(out_fill, np.int32).copy()
    _ok(lib().mpf_probe_column(_ptr(Cm, i32p), rows, Cm.shape[1], col, _ptr(out, i32p), out.shape[0]), "mpf_probe_column")
    return out


def _pub(a, keep, ranges):
    """Fill the three publication ranges of a probe struct; returns the destination arrays."""
    dst = []
    for k in range(3):
        s = _arr(ranges[k] if ranges is not None and k < len(ranges) else [], np.uint32)
        d = np.full(max(len(s), 1), 0xDEADBEEF, np.uint32)
        keep += [s, d]
        a.pub_src[k], a.pub_dst[k], a.pub_words[k] = _ptr(s, u32p), _ptr(d, u32p), len(s)
        dst.append(d[:len(s)])
    return dst


def events(case, route, B, fixed=False, crow=True, ev_cap=None, n_idx=None, clamp_rt=False, cut=None, ranges=None, h_ev_cap=0):
    """The event extraction of an EventCase (make_event_case).  route 0 = launch_ufb_events, 1 = launch_ufb_events_publish.
    Returns a dict: count, ev [min(count, ev_cap)][3], and for route 1 h_flag, done, dst (three arrays), h_ev."""
    n = case["n_idx"] if n_idx is None else n_idx
    info, cost = _arr(case["info"], np.uint32), _arr(case["cost"], np.uint32)
    thr, home = _arr(case["thr"], np.uint32), _arr(case["home"], np.uint32)
    cr = _arr(case["crow"], np.uint32) if crow else None
    Cm = _arr(case["C_crow"] if crow else case["C_direct"], np.int32)
    rt, best = _arr(case["rt"], np.int32), _arr(case["best"], np.uint32)
    cap = n * B + 1 if ev_cap is None else ev_cap
    ev, cnt = np.zeros((max(cap, 1), 3), np.uint32), np.zeros(1, np.uint32)
    h_ev, h_flag, done = np.zeros((max(h_ev_cap, 1), 3), np.uint32), np.zeros(4, np.uint32), np.full(1, 7, np.uint32)
    a = _Events()
    keep = []
    a.route, a.info, a.cost, a.thr, a.home, a.crow = route, _ptr(info, u32p), _ptr(cost, u32p), _ptr(thr, u32p), _ptr(home, u32p), _ptr(cr, u32p)
    a.C, a.rt, a.best = _ptr(Cm, i32p), _ptr(rt, i32p), _ptr(best, u32p)
    a.n_idx, a.n_parts, a.c_rows, a.Bp, a.B = n, len(thr), Cm.shape[0], Cm.shape[1], B
    a.fixed_bound, a.clamp_rt, a.have_cut, a.cut = int(fixed), int(clamp_rt), int(cut is not None), 0 if cut is None else cut
    a.ev, a.ev_cap, a.ev_count = _ptr(ev, u32p), cap, _ptr(cnt, u32p)
    dst = _pub(a, keep, ranges)
    a.h_ev, a.h_ev_cap, a.h_flag, a.done = _ptr(h_ev, u32p), h_ev_cap, _ptr(h_flag, u32p), _ptr(done, u32p)
    _ok(lib().mpf_probe_events(C.byref(a)), "mpf_probe_events")
    count = int(cnt[0])
    return {"count": count, "ev": ev[:min(count, cap)], "h_flag": h_flag, "done": int(done[0]), "dst": dst, "h_ev": h_ev[:min(count, h_ev_cap)]}


def mid(kind, Cm, c_words, info, self_idx, code, ev_count=99, cost=None, home=None, plan_end=None, cut=0x12345678, ranges=None):
    """kind 0 launch_ufb_mid, 1 launch_ufb_prep, 2 launch_ufb_self.  Returns dict C, info, ev_count, cut, h_flag, done, dst."""
    Cm, info, idx = _arr(Cm, np.int32).copy(), _arr(info, np.uint32).copy(), _arr(self_idx, np.uint32)
    cost_a = _arr(cost if cost is not None else [], np.uint32)
    home_a, pend = _arr(home if home is not None else [], np.uint32), _arr(plan_end if plan_end is not None else [], np.uint32)
    evc, cutw, h_flag, done = np.full(1, ev_count, np.uint32), np.full(1, cut, np.uint32), np.zeros(4, np.uint32), np.full(1, 7, np.uint32)
    a = _Mid()
    keep = []
    a.kind, a.C, a.c_total, a.c_words = kind, _ptr(Cm, i32p), Cm.size, c_words
    a.info, a.self_idx, a.n_self, a.code, a.ev_count = _ptr(info, u32p), _ptr(idx, u32p), len(idx), code, _ptr(evc, u32p)
    a.cost, a.home, a.plan_end, a.n_idx, a.n_parts, a.cut = _ptr(cost_a, u32p), _ptr(home_a, u32p), _ptr(pend, u32p), info.shape[0], len(home_a), _ptr(cutw, u32p)
    dst = _pub(a, keep, ranges)
    a.h_flag, a.done = _ptr(h_flag, u32p), _ptr(done, u32p)
    _ok(lib().mpf_probe_mid(C.byref(a)), "mpf_probe_mid")
    return {"C": Cm, "info": info, "ev_count": int(evc[0]), "cut": int(cutw[0]), "h_flag": h_flag, "done": int(done[0]), "dst": dst}


# ------------------------------------------------------------------------------------------------ the references
def unpack_bits(masks):
    """[rows][Wp] uint32 -> [rows][32 Wp] 0/1 (bit j of word i = site 32 i + j)."""
    m = np.ascontiguousarray(masks, dtype="<u4")
    return np.unpackbits(m.view(np.uint8), axis=1, bitorder="little")


def ref_product(masks, Wsite):
    """bits x Wsite in float64 (BLAS); exact while every sum stays below 2^53.  Wsite [sites][cols]."""
    bits = unpack_bits(masks)[:, :Wsite.shape[0]].astype(np.float64)
    out = bits @ np.asarray(Wsite, np.float64)
    assert np.abs(out).max(initial=0) < 2.0 ** 53
    return np.rint(out).astype(np.int64)


def ref_product_int(masks, Wsite):
    return unpack_bits(masks)[:, :Wsite.shape[0]].astype(np.int64) @ np.asarray(Wsite, np.int64)


def site_weights(src, first, cur, n_sites):
    """[n_sites][n_cols]: the weight of pattern p at site first[p], where first[p] >= 0 and cur[p] > 0 (distinct sites)."""
    src, first, cur = np.asarray(src, np.int64), np.asarray(first), np.asarray(cur)
    ok = (first >= 0) & (cur > 0)
    assert len(set(first[ok].tolist())) == int(ok.sum()), "two patterns on one site"
    W = np.zeros((n_sites, src.shape[0]), np.int64)
    W[first[ok]] = src[:, ok].T
    return W


def ref_chain(masks, src, first, cur):
    """C[row][col] = sum over patterns p with first[p] >= 0 and cur[p] > 0 of bit(mask[row], first[p]) * src[col][p]."""
    return ref_product(masks, site_weights(src, first, cur, 32 * np.asarray(masks).shape[1]))


def ref_weighted(vals, W):
    """vals [rows][npat] x W [n_cols][npat] -> [rows][n_cols]."""
    return np.asarray(vals, np.int64) @ np.asarray(W, np.int64).T


def ref_planes(vals, K, planes_in):
    """planes_in with bit i of word w of plane k, row r = bit k of vals[r][32 w + i] for the words that hold a pattern's 64-tile."""
    vals = np.asarray(vals, np.uint16)
    out = np.array(planes_in, np.uint32)
    rows, npat = vals.shape
    nw = 2 * ((npat + 63) // 64)
    padded = np.zeros((rows, 32 * nw), np.uint8)
    for k in range(K):
        padded[:, :npat] = (vals >> k) & 1
        out[k, :rows, :nw] = np.packbits(padded, axis=1, bitorder="little").view("<u4")
    return out


def ref_join_masks(vec, ops):
    vec = np.asarray(vec, np.uint32)
    return np.stack([~np.bitwise_or.reduce(vec[a] & vec[b], axis=0) for a, b, _o, _p in np.asarray(ops).tolist()]).astype(np.uint32)


def ref_scores(case, crow, n_idx=None):
    """[n_idx][Bp] uint32 scores by ufb_score's rule, NONE where the index takes no part: a home slot never does; the current
    tree's slot scores R_T; a candidate takes part iff cost < thr[part] and scores R_T - C[row(home[part])] + C[row(i)], where
    row() is crow[] if given and the index's own mask row (info[i][0]; the home index itself for the home) otherwise."""
    info, cost, thr, home = case["info"], case["cost"], case["thr"], case["home"]
    Cm = np.asarray(case["C_crow"] if crow else case["C_direct"], np.int64)
    rt = np.asarray(case["rt"], np.int64)
    n = case["n_idx"] if n_idx is None else n_idx
    sc = np.full((n, Cm.shape[1]), NONE, np.int64)
    for i in range(n):
        row, part = int(info[i][0]), int(info[i][1])
        if part == SKIP:
            continue
        if part == SELF:
            sc[i] = rt & 0xFFFFFFFF
            continue
        if int(cost[i]) >= int(thr[part]):
            continue
        h = int(home[part])
        rc, rh = (int(case["crow"][i]), int(case["crow"][h])) if crow else (row, h)
        sc[i] = (rt - Cm[rh] + Cm[rc]) & 0xFFFFFFFF
    return sc


def ref_events(case, B, fixed=False, crow=True, n_idx=None, clamp_rt=False, cut=None, scores=None):
    """Per sample, the indices in order: an event is score <= run; then run = score unless the bound is fixed.
    Returns ([count][3] rows (idx, b, s) in sorted order, count).  scores: ref_scores(case, crow) where the caller has them."""
    n = case["n_idx"] if n_idx is None else n_idx
    if cut is not None:
        n = min(n, cut)
    sc = (ref_scores(case, crow, n) if scores is None else scores[:n])[:, :B]
    run = np.asarray(case["best"], np.int64)[:B].copy()
    if clamp_rt:
        run = np.minimum(run, np.asarray(case["rt"], np.int64)[:B] & 0xFFFFFFFF)
    ii, bb, ss = [], [], []
    for i in range(n):
        s = sc[i]
        hit = (s != NONE) & (s <= run)
        b = np.nonzero(hit)[0]
        if len(b):
            ii.append(np.full(len(b), i))
            bb.append(b)
            ss.append(s[b])
        if not fixed:
            run = np.where(hit, s, run)
    out = np.stack([np.concatenate(x) for x in (ii, bb, ss)], axis=1).astype(np.int64) if ii else np.zeros((0, 3), np.int64)
    return out, len(out)


def ref_cut(info, cost, home, plan_end, n_idx):
    """Smallest plan_end over the parts that hold a candidate cheaper than the part's home; n_idx when there is none."""
    cut = n_idx
    for k in range(n_idx):
        part = int(info[k][1])
        if part >= SELF:
            continue
        if int(cost[k]) < int(cost[int(home[part])]):
            cut = min(cut, int(plan_end[part]))
    return cut


def sorted_events(ev):
    """[n][3] events in (idx, b, s) order (the device stores them in any order); duplicates stay."""
    a = np.asarray(ev, np.int64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def event_set(ev):
    return {(int(i), int(b), int(s)) for i, b, s in np.asarray(ev).reshape(-1, 3).tolist()}


# ------------------------------------------------------------------------------------------------ inputs
def make_event_case(n_idx, B, Bp, seed, part_len=11):
    """Index space as the scan lays it out: every part is [current tree's slot][candidates ...][home slot]; scores from a narrow
    range around a level that steps down (ties with the running minimum are common, new minima keep coming); some costs at and
    above thr; the padding columns of C, rt, best hold noise.
    Two forms of the same product: C_direct (row = info[i][0], the home's row = its index) and C_crow (row = crow[i])."""
    rng = np.random.default_rng(seed)
    info = np.zeros((n_idx, 2), np.uint32)
    cost = rng.integers(95, 106, n_idx).astype(np.uint32)
    home, thr, plan_end = [], [], []
    i = 0
    while i < n_idx:
        ln = min(n_idx - i, int(rng.integers(3, part_len + 1)))
        p = len(home)
        h = i + ln - 1                                     # (a part of one index is its home slot alone)
        info[i:i + ln, 1] = p
        info[i:i + ln, 0] = np.arange(i, i + ln)           # mask row = index (direct form)
        if ln >= 3:
            info[i] = (0, SELF if rng.random() < 0.7 else SKIP)
        info[h] = (h, SKIP) if ln > 1 else (0, SELF)       # (a lone index: the current tree's slot, its part stays empty)
        home.append(h)
        thr.append(int(rng.choice([100, 101, 106, 95])))   # at, above and below the costs' range
        plan_end.append(i + ln)
        i += ln
    perm = rng.permutation(n_idx).astype(np.uint32)       # crow: any one-to-one map of indices to rows
    C_direct = np.zeros((n_idx, Bp), np.int32)
    C_direct[:, :] = rng.integers(1000, 1004, (n_idx, Bp))
    # the candidates' level steps down along the scan, so that new minima keep coming -- at the last and the first indices of the
    # extraction's slices (16), passes and chunks (256) above all, where a prefix that is off by one index shows -- and here and there
    steps = np.zeros(n_idx, np.int32)
    edges = [e + d for e in (16, 32) + tuple(range(256, n_idx + 2, 256)) for d in (-1, 0, 1)]
    steps[np.array([e for e in edges if e < n_idx], dtype=np.int64)] = 1
    steps[rng.random(n_idx) < 0.01] = 1
    level = -np.cumsum(steps)
    level[np.array(home)] = 0
    C_direct += level[:, None].astype(np.int32)
    C_direct[:, B:] = rng.integers(-2 ** 31, 2 ** 31 - 1, (n_idx, Bp - B))
    C_crow = np.zeros_like(C_direct)
    C_crow[perm] = C_direct
    rt = rng.integers(5000, 5003, Bp).astype(np.int32)
    best = rng.integers(4999, 5004, Bp).astype(np.uint32)
    rt[B:] = rng.integers(-2 ** 31, 2 ** 31 - 1, Bp - B)
    best[B:] = rng.integers(0, 2 ** 32 - 1, Bp - B)
    return {"n_idx": n_idx, "info": info, "cost": cost, "thr": np.array(thr, np.uint32), "home": np.array(home, np.uint32),
            "plan_end": np.array(plan_end, np.uint32), "crow": perm, "C_direct": C_direct, "C_crow": C_crow, "rt": rt, "best": best}


def distinct_weights(n_sites, n_cols, rng, top=127):
    """[n_cols][n_sites] uint16 in 1..top, no two alike within a 127-run where top allows: a permutation of k or of columns shows."""
    base = (np.arange(n_sites)[None, :] * 31 + np.arange(n_cols)[:, None] * 17 + int(rng.integers(0, top))) % top + 1
    return base.astype(np.uint16)
