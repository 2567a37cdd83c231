"""Witness of the tracked NNI climb under the tracker's optional update rules and on a sample-sharded tracker -- TEST
INFRASTRUCTURE ONLY.

The climbs are those of tests/nni_bb_witness.py (Fitch) and tests/nni_snk_bb_witness.py (weighted), taken by import: which trees
reach saveCurrentTree, in which order, each with which row of per-pattern lengths.  What happens to a tree once it is there is
restated HERE, from the reference text and apart from oracle/search_slow.py's restatement (tests/test_nni_bb_rules_witness.py
feeds both the same offers and compares them):

    -storetrees                 iqtree.cpp:3302-3351   RuleBooks._enter
    -mulhits                    iqtree.cpp:3498-3536   RuleBooks._offer_mulhits
    -mulhits -topboot N         iqtree.cpp:3538-3583   RuleBooks._offer_topboot
    -distinct_iter_top_boot k   iqtree.cpp:3587-3680   RuleBooks._offer_distinct
    default                     iqtree.cpp:3687-3732   RuleBooks._offer_default

The structure differs from SlowSearch.save_current_tree on purpose: one call is cut into `_enter` (ratchet length, topology
look-up, cut-off: -> the tree's index or nothing), the OFFERS (sample, rell) of the tree's row, and one `_offer_*` per rule; the
tree's string is a lazily resolved `_Str` object as in the reference (empty until somebody needs it).

Two shards: `shards = [ids_0, ids_1]` makes every call's offers in two `ShardColumns`, each of which holds the weights of its
own samples only and knows nothing of the other; what they hand back is merged in sample order, as the ranks' exchanged events
are, and replayed.  `shard_steps[(climb, step)]` remembers which shards contributed an offer that changed some sample's books.
"""
import numpy as np

from nni_bb_witness import NniBbWitness
from nni_snk_bb_witness import SnkNniBbWitness

class ShardColumns:
    """one rank's share of the samples: rell of a row of per-pattern lengths under each of ITS samples"""

    def __init__(self, samples, ids):
        self.ids = [int(b) for b in ids]
        self.w = np.asarray(samples, dtype=np.int64)[self.ids]

    def offers(self, row):
        r = self.w @ np.asarray(row, dtype=np.int64)
        return [(b, -float(v)) for b, v in zip(self.ids, r.tolist())]


class _Str:
    """tree_str of one saveCurrentTree call: "" until the first sample that needs it (or -storetrees at the top)"""

    def __init__(self, books, tree_index):
        self.books, self.index, self.set = books, tree_index, False

    def need(self):
        if not self.set:                                                 # treels.find / treels[tree_str] = treels_logl.size() - 1
            bk = self.books
            self.index = bk.treels.setdefault(bk.splits(bk.back), len(bk.treels_logl) - 1)
            self.set = True
        return self.index


class RuleBooks:
    """saveCurrentTree, restated.  Mixed in FRONT of a witness that derives from SlowSearch: uses its state arrays (same names, so
    that the two restatements can be compared field by field), its `splits`, `pattern_lengths`, `draw`; replaces save_current_tree"""

    shards = None                                   # None | [ids_0, ids_1]
    cur_step = 0
    cur_climb = 0                                   # (the driver counts the climbs on one tracker)

    def rules_init(self):
        self.offers_rejected_same_iter = 0          # -distinct: accepted by the threshold test, but this iteration has a better one
        self.displaced = 0                          # -topboot: a full list dropped its last entry
        self.dup_improved = 0                       # -storetrees: a known topology came back with a better length ...
        self.dup_improved_past_cut = 0              # ... of these, with a length that fails the cut-off in force
        self.new_failed_cut = 0                     # a NEW topology that failed the cut-off (never stored, with or without -storetrees)
        self.shard_steps = {}
        self.live_calls = 0                         # calls that got past the first lines (not a climb -no_hclimb1_bb keeps out)
        self._cols = None

    # ---- the top of the call: -> _Str or None
    def _enter(self, cur_logl):
        fails = self.cutoff != 0.0 and cur_logl <= self.cutoff - 1e-4
        if self.store_trees:
            key = self.splits(self.back)
            at = self.treels.get(key)
            if at is not None:
                self.duplicates += 1
                if cur_logl <= self.treels_logl[at] + 1e-4:
                    return None
                self.treels_logl[at] = cur_logl
                self.dup_improved += 1
                self.dup_improved_past_cut += bool(fails)
                s = _Str(self, at)
                s.set = True
                return s
        if fails:
            self.new_failed_cut += 1
            return None
        s = _Str(self, len(self.treels_logl))
        if self.store_trees:
            self.treels[key] = s.index
            s.set = True
        self.treels_logl.append(cur_logl)
        return s

    def _keep_topology(self, t):
        self.topologies.setdefault(t, list(self.back))

    # ---- the rules: one (sample, rell) each; True if the sample's books changed
    def _offer_default(self, b, rell, s, cur_logl):
        best = self.boot_logl[b]
        changed = False
        if rell > best + self.eps or (rell > best - self.eps and self._tie(1.0 / (self.boot_counts[b] + 1))):
            t = s.need()
            if rell > best:
                self.boot_counts[b] = 1
            if self.cutoff_from_btrees:
                self.boot_tree_orig_logl[b] = int(cur_logl)
            self.boot_logl[b] = max(best, rell)
            self.boot_trees[b] = t
            self._keep_topology(t)
            changed = True
        if rell == self.boot_logl[b]:
            self.boot_counts[b] += 1
        return changed

    def _offer_mulhits(self, b, rell, s, cur_logl):
        if rell < self.boot_logl[b]:
            return False
        t = s.need()
        if rell > self.boot_logl[b]:
            self.boot_sets[b] = set()
            self.boot_logl[b] = rell
        if self.cutoff_from_btrees and cur_logl > self.boot_tree_orig_logl[b]:
            self.boot_tree_orig_logl[b] = int(cur_logl)
        if t in self.boot_sets[b]:
            return False
        self.boot_sets[b].add(t)
        self.largest_set = max(self.largest_set, len(self.boot_sets[b]))
        self._keep_topology(t)
        return True

    def _offer_topboot(self, b, rell, s, cur_logl):
        N, lst = self.topboot, self.boot_top[b]
        if not (len(lst) < N or rell > self.boot_threshold[b]):
            return False
        t = s.need()
        if t != len(self.treels_logl) - 1:                               # not newly added
            return False
        if len(lst) < N:
            where = next((i for i, e in enumerate(lst) if e[1] < rell), len(lst))
            lst.insert(where, (t, int(rell)))
            self.boot_threshold[b] = self.boot_threshold[b] if self.boot_threshold[b] < rell else int(rell)
        elif rell > self.boot_threshold[b]:
            lst.pop()
            self.displaced += 1
            where = next((i for i, e in enumerate(lst) if e[1] < rell), len(lst))
            lst.insert(where, (t, int(rell)))
            self.boot_threshold[b] = lst[N - 1][1]
        else:
            return False
        self._keep_topology(t)
        return True

    def _offer_distinct(self, b, rell, s, cur_logl):
        k, thr = self.distinct, self.boot_threshold[b]
        if rell >= thr:
            self.boot_counts[b] += 1
        if not (rell > thr or (rell == thr and self._tie(k * 1.0 / self.boot_counts[b]))):
            return False
        if rell > self.boot_logl[b]:
            self.boot_counts[b] = 1
        t = s.need()
        if self.cutoff_from_btrees:
            self.boot_tree_orig_logl[b] = int(cur_logl)
        self.boot_trees[b] = t
        self.boot_logl[b] = max(self.boot_logl[b], rell)
        self._keep_topology(t)
        lst, its = self.boot_top[b], self.boot_top_iter[b]
        n_in = min(k, len(its))
        if any(lst[c][0] == t for c in range(n_in)):
            return True
        c = 0
        while c < n_in and its[c] != self.cur_it:
            c += 1
        if c < n_in:                                                     # this iteration has its representative
            if rell > lst[c][1]:
                lst[c] = (t, int(rell))
            else:
                self.offers_rejected_same_iter += 1
        elif n_in < k:
            its.append(self.cur_it)
            lst.append((t, int(rell)))
        else:
            worst = 0
            for d in range(1, n_in):
                if lst[d][1] < lst[worst][1]:
                    worst = d
            lst[worst] = (t, int(rell))
            its[worst] = self.cur_it
        self.boot_threshold[b] = min(e[1] for e in lst)
        return True

    def _tie(self, bound):
        self.ufb_draws += 1
        return self.draw() <= bound

    # ---- the call
    def save_current_tree(self, cur_logl):
        if not self.bb_on:
            return
        self.live_calls += 1
        if self.ratchet:                                                 # :3283-3294, from _pattern_pars as the caller left it
            cur_logl = -float(int((self.pattern_pars * self.orig * self.inf).sum()))
        s = self._enter(cur_logl)
        if s is None:
            return
        self.pattern_pars = self.pattern_lengths(self.back)
        if self._cols is None:
            groups = self.shards if self.shards is not None else [range(self.samples.shape[0])]
            self._cols = [ShardColumns(self.samples, ids) for ids in groups]
        offers = sorted((o + (r,) for r, col in enumerate(self._cols) for o in col.offers(self.pattern_pars)), key=lambda o: o[0])
        if self.distinct and not self.mulhits:
            rule = self._offer_distinct
        elif self.mulhits and self.topboot:
            rule = self._offer_topboot
        elif self.mulhits:
            rule = self._offer_mulhits
        else:
            rule = self._offer_default
        for b, rell, rank in offers:
            if rule(b, rell, s, cur_logl):
                self.shard_steps.setdefault((self.cur_climb, self.cur_step), set()).add(rank)


class NniBbRulesWitness(RuleBooks, NniBbWitness):
    def __init__(self, *a, **kw):
        NniBbWitness.__init__(self, *a, **kw)
        self.rules_init()

    def book(self, length, kind, step):
        self.cur_step = step
        NniBbWitness.book(self, length, kind, step)


class SnkNniBbRulesWitness(RuleBooks, SnkNniBbWitness):
    def __init__(self, *a, **kw):
        SnkNniBbWitness.__init__(self, *a, **kw)
        self.rules_init()

    def book(self, length, kind, edge):
        self.cur_step = self.step
        SnkNniBbWitness.book(self, length, kind, edge)


def set_rule(w, rule, arg=0, store=False):
    """rule: "default" | "mulhits" | "topboot" | "distinct"; store: -storetrees on top"""
    w.mulhits = rule in ("mulhits", "topboot")
    w.topboot = arg if rule == "topboot" else 0
    w.distinct = arg if rule == "distinct" else 0
    w.store_trees = bool(store)


def shard_ids(B, how):
    """two ranks' samples: "interleaved" (rank, rank + 2, ...) or "contiguous" (the first half, the rest)"""
    if how == "interleaved":
        return [list(range(0, B, 2)), list(range(1, B, 2))]
    h = (B + 1) // 2
    return [list(range(0, h)), list(range(h, B))]


def make(fx, tie_seed, samples, root_taxon=1, keep_all=False):
    inf = np.ones(len(fx["weights"]), dtype=bool) if keep_all else np.asarray(fx["informative"], dtype=bool)
    return NniBbRulesWitness(fx["codes_np"], fx["weights_np"], fx["datatype"], inf, tie_seed, samples, root_taxon)


def make_snk(fx, cost, tie_seed, samples, root_taxon=1):
    return SnkNniBbRulesWitness(fx["codes_np"], fx["weights_np"], fx["datatype"], cost, tie_seed, samples, root_taxon)
