// ufboot_common.hpp -- what the translation units of the online UFBoot bookkeeping share (host/ufboot*.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <pthread.h>
#include <sched.h>
#include "../csrc/engine.hpp"
#include "lcg_block.hpp"
#include "simd_util.hpp"
#include "spr_rule.hpp"
#include "ufb_cutoff.hpp"

namespace mpf {

#define UCHK(expr)                                                                                   \
  do {                                                                                               \
    hipError_t e__ = (expr);                                                                         \
    if (e__ != hipSuccess) { set_error(std::string(#expr) + ": " + hipGetErrorString(e__)); return MPF_E_HIP; } \
  } while (0)

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
static inline bool ufb_trace_env() { static const bool on = std::getenv("MPF_UFB_TRACE") != nullptr; return on; }
static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// events into replay order: by scan output index, then by sample.  The current tree, booked once per prune-node visit, ties
// with every sample it is the best tree of -- millions of events per sweep -- so large batches take two stable counting
// passes (sample, then index) instead of a comparison sort.
static inline void sort_events(std::vector<UfbEvent> &ev, std::vector<UfbEvent> &tmp, std::vector<uint32_t> &count, uint32_t n_idx, uint32_t n_samples)
{
  const size_t n = ev.size();
  if (n < 512) {
    std::sort(ev.begin(), ev.end(), [](const UfbEvent &x, const UfbEvent &y) { return x.idx != y.idx ? x.idx < y.idx : x.b < y.b; });
    return;
  }
  tmp.resize(n);
  auto pass = [&](const std::vector<UfbEvent> &src, std::vector<UfbEvent> &dst, uint32_t nkeys, bool by_idx) {
    count.assign((size_t)nkeys + 1, 0u);
    for (const UfbEvent &e : src) count[(size_t)(by_idx ? e.idx : e.b) + 1]++;
    for (size_t k = 1; k <= nkeys; k++) count[k] += count[k - 1];
    for (const UfbEvent &e : src) dst[count[by_idx ? e.idx : e.b]++] = e;
  };
  uint32_t max_idx = 0;
  for (const UfbEvent &e : ev) max_idx = std::max(max_idx, e.idx);     // (a sharded run's merged events: other ranks' indices too)
  pass(ev, tmp, n_samples, false);
  pass(tmp, ev, std::max(n_idx, max_idx + 1u), true);
}

// the -distinct_iter_top_boot block of saveCurrentTree for one (tree, sample); tree_index / looked_up: the call's tree string
// state (resolved through `lookup` at the first acceptance); true if some list or boot_trees entry now names tree_index
template <class Lookup>
bool Engine::ufb_distinct_offer(uint32_t b, int32_t rell, int64_t &tree_index, bool &looked_up, Lookup lookup)
{
  UfbState &u = *ufb_;
  auto &top = u.top[b];
  auto &its = u.top_iter[b];
  int32_t &thr = u.top_thr[b];
  const int k = u.distinct;
  if (rell >= thr) u.boot_counts[b]++;                                      // :3589-3591
  bool take = rell > thr;
  if (!take && rell == thr) {                                               // :3593-3595, the draw only on a tie
    u.draws++;
    take = tie_draw() <= (double)k * 1.0 / (double)u.boot_counts[b];
  }
  if (!take) return false;
  uint32_t &bs = u.boot_score[b];
  const uint32_t len = (uint32_t)(-(int64_t)rell);
  if (len < bs) u.boot_counts[b] = 1;                                       // :3598-3600
  if (u.cut_btrees) u.boot_orig[b] = u.cur_logl_now;                                          // :3617-3619
  if (!looked_up) { tree_index = lookup(tree_index); looked_up = true; }
  bool named = false;
  auto ref = [&](int64_t t) { u.refs[(size_t)t]++; named = true; };
  auto unref = [&](int64_t t) { if (--u.refs[(size_t)t] == 0) u.store.erase(t); };
  int64_t &bt = u.boot_trees[b];
  if (bt != tree_index) {                                                   // :3620
    ref(tree_index);
    if (bt >= 0) unref(bt);
    bt = tree_index;
  }
  if (len < bs) bs = len;                                                   // :3621 max()
  const int t = std::min(k, (int)its.size());
  for (int c = 0; c < t; c++) if (top[(size_t)c].first == tree_index) return named;      // :3627-3634 tree exists
  int c = 0;
  for (; c < t; c++)
    if (its[(size_t)c] == u.cur_it) {                                       // :3637-3645 this iteration's representative
      if (rell > top[(size_t)c].second) {
        ref(tree_index);
        unref(top[(size_t)c].first);
        top[(size_t)c] = std::make_pair(tree_index, rell);
      }
      break;
    }
  if (c == t && t < k) {                                                    // :3648-3651
    its.push_back(u.cur_it);
    top.push_back(std::make_pair(tree_index, rell));
    ref(tree_index);
  } else if (c == t && t == k) {                                            // :3654-3667 replace the worst
    int worst = 0;
    for (int d = 1; d < t; d++) if (top[(size_t)d].second < top[(size_t)worst].second) worst = d;
    ref(tree_index);
    unref(top[(size_t)worst].first);
    top[(size_t)worst] = std::make_pair(tree_index, rell);
    its[(size_t)worst] = u.cur_it;
  }
  thr = top[0].second;                                                      // :3670-3675
  for (size_t d = 1; d < top.size(); d++) thr = std::min(thr, top[d].second);
  return named;
}

// The update rule of one booked tree for one sample (b, score s) -- iqtree.cpp:3684-3731 and its -mulhits / -topboot /
// -distinct_iter_top_boot variants (:3498-3680): shared by the events the device extracted and by the current tree's own
// bookings the host walks through itself.  lookup(tree_index, cand_code) = treels.find(tree_str) / treels[tree_str] = tree_index
// (:3500-3514, :3689-3707): a topology that some sample accepted before keeps the index of that first tree.
template <class Lookup>
void Engine::ufb_one_event(const uint32_t b, const uint32_t s, int64_t &tree_index, bool &looked_up, const uint32_t cand_code, Lookup lookup, const UfbDeferCtx &dc)
{
  UfbState &u = *ufb_;
  uint32_t &bs = u.boot_score[b];
  if (u.distinct && !u.mulhits) {
    if (ufb_distinct_offer(b, -(int32_t)s, tree_index, looked_up, [&](int64_t ti) { return lookup(ti, cand_code); }) &&
        (u.pending.empty() || u.pending.back().tree_index != tree_index)) u.pending.push_back(UfbState::Pending{tree_index, cand_code});
    return;
  }
  if (u.mulhits && u.topboot) {
    // iqtree.cpp:3542-3585: the sample's list is not full yet, or the tree beats its threshold
    const int32_t rell = -(int32_t)s;
    if ((int)u.top[b].size() < u.topboot || rell > u.top_thr[b]) {
      const int64_t newest = (int64_t)u.treels.size() - 1;
      if (!looked_up) { tree_index = lookup(tree_index, cand_code); looked_up = true; }
      if (ufb_topboot_offer(b, rell, tree_index, tree_index == newest) &&
          (u.pending.empty() || u.pending.back().tree_index != tree_index)) u.pending.push_back(UfbState::Pending{tree_index, cand_code});
    }
    return;
  }
  if (u.mulhits) {
    // iqtree.cpp:3498-3540: rell >= boot_logl (an event is exactly that); no draw, boot_counts untouched
    if (s > bs) return;
    if (!looked_up) { tree_index = lookup(tree_index, cand_code); looked_up = true; }       // :3500-3514
    std::set<int64_t> &hs = u.hit_sets[b];
    if (s < bs) {                                               // :3516-3519
      for (int64_t t : hs) if (--u.refs[(size_t)t] == 0) u.store.erase(t);
      hs.clear();
      bs = s;
    }
    if (u.cut_btrees && u.cur_logl_now > u.boot_orig[b]) u.boot_orig[b] = u.cur_logl_now;     // :3523-3527
    if (hs.insert(tree_index).second) {                         // :3530-3533
      u.refs[(size_t)tree_index]++;
      if (u.pending.empty() || u.pending.back().tree_index != tree_index) u.pending.push_back(UfbState::Pending{tree_index, cand_code});
    }
    return;
  }
  bool accept = false;
  if (s < bs) accept = true;                                    // rell > boot_logl + epsilon (:3686)
  else if (s == bs) {                                           // rell > boot_logl - epsilon: tie, draw (:3687-3688)
    ++*(dc.draws ? dc.draws : &u.draws);
    accept = tie_draw() <= 1.0 / (double)(u.boot_counts[b] + 1);
  }
  if (accept && u.cut_btrees) u.boot_orig[b] = u.cur_logl_now;                  // :3716-3718
  if (accept && dc.on) {
    // (deferred: nothing of the state a pipelined climb's worker thread owns -- refs, boot_trees, store, topo_index -- is touched)
    u.log.push_back(UfbState::LogEntry{b, cand_code, tree_index, dc.cur_plan});
    *dc.log_open = true;
    if (dc.moot && cand_code != 0xFFFFFFFFu && dc.moot->flag[b]) { dc.moot->flag[b] = 0; dc.moot->n_set--; }   // (it points elsewhere now)
    if (dc.moot && s < bs) dc.moot->n_le = -1;
    if (s < bs) { u.boot_counts[b] = 1; bs = s; }              // :3710-3719
  } else if (accept) {
    // the tree "string" (:3689-3707): looked up once per booked tree; the topology itself is remembered as
    // (prune node, candidate) and materialised after this prune node's scan only if some sample still points to it
    if (!looked_up) { tree_index = lookup(tree_index, cand_code); looked_up = true; }
    if (u.pending.empty() || u.pending.back().tree_index != tree_index) u.pending.push_back(UfbState::Pending{tree_index, cand_code});
    if (s < bs) { u.boot_counts[b] = 1; bs = s; }              // :3710-3719
    int64_t &bt = u.boot_trees[b];
    if (bt != tree_index) {
      if (bt >= 0 && --u.refs[(size_t)bt] == 0) u.store.erase(bt);
      u.refs[(size_t)tree_index]++;
      bt = tree_index;                                          // :3720
    }
  }
  if (s == bs) u.boot_counts[b]++;                              // :3728-3730
}

// One tree arriving at saveCurrentTree with length cur_len: its index in treels_logl, or -1 when nothing is booked.
// Default: the cut-off test, then a new index (iqtree.cpp:3343-3348).  -storetrees: looked up by topology first
// (:3302-3341; key(cand_code) = its canonical form); one met before is skipped unless the length improved on the recorded one,
// and then it goes on under its old index without the cut-off test.  grow_refs = false: a pipelined climb's worker thread owns the
// reference counts and sizes them itself.
template <class KeyFn>
int64_t Engine::ufb_book_tree(uint32_t cur_len, bool passes_cut, uint32_t cand_code, bool store_trees, KeyFn key, bool grow_refs)
{
  UfbState &u = *ufb_;
  if (store_trees) {
    const std::string &k = key(cand_code);
    auto it = u.topo_index.find(k);
    if (it != u.topo_index.end()) {
      u.duplicates++;
      if (cur_len >= u.treels[(size_t)it->second]) return -1;
      u.treels[(size_t)it->second] = cur_len;
      return it->second;
    }
    if (!passes_cut) return -1;
    u.topo_index.emplace(k, (int64_t)u.treels.size());
  } else if (!passes_cut) return -1;
  u.treels.push_back(cur_len);
  if (grow_refs) u.refs.push_back(0);
  return (int64_t)u.treels.size() - 1;
}

// ---- the event extraction of a neighbourhood that is not the SPR scan (the tracked NNI step, host/nni.cpp; the tracked TBR sweep,
// host/tbr.cpp)
// One step's event extraction.  Output indices: 0 = the current tree (offered on the host), 1 + c = candidate c, behind them the
// home slots; part[idx] = the part of a candidate (0xFFFFFFFF: no candidate), home[part] = its home slot, crow[idx] = the row of C
// an index reads (0xFFFFFFFF: none), pass[c]: candidate c takes part (under -storetrees every one does: the replay decides).  sel_rows (or nullptr): the mask rows a compact product
// multiplies, handed to product(rows_p, device copy) -- which runs here unless the caller has C already.  events: in replay order.
// staging: thr[n_parts] | home[n_parts] | best[Bp] | crow[n_idx] | cost[n_idx] | (even) info[n_idx] as pairs | sel[rows_p] | event counter
template <class Product>
int Engine::nni_extract_events(uint32_t n_idx, const std::vector<uint32_t> &home, const std::vector<uint32_t> &part, const std::vector<uint32_t> &crow,
                               const std::vector<uint8_t> &pass, const std::vector<uint32_t> *sel_rows, int rows_p, bool have_C, Product product,
                               std::vector<UfbEvent> &events)
{
  UfbState &u = *ufb_;
  const size_t n_parts = home.size();
  const size_t o_home = n_parts, o_best = 2 * n_parts, o_crow = o_best + (size_t)u.Bp, o_cost = o_crow + n_idx;
  const size_t o_info = (o_cost + n_idx + 1) & ~(size_t)1, o_sel = o_info + 2 * (size_t)n_idx, o_cnt = o_sel + (sel_rows ? (size_t)rows_p : 0);
  UCHK(u.h_small.reserve(o_cnt + 4));
  UCHK(u.thr.reserve(o_cnt + 4));
  uint32_t *sm = u.h_small.p;
  std::memset(sm, 0, (o_cnt + 1) * sizeof(uint32_t));           // (padding columns of best: 0 -> never an event; padding rows multiply mask row 0)
  for (size_t i = 0; i < n_parts; i++) { sm[i] = 1u; sm[o_home + i] = home[i]; }            // a candidate takes part iff cost < 1
  for (int c2 = 0; c2 < u.Bl; c2++) sm[o_best + (size_t)c2] = ufb_event_bound((uint32_t)u.ids[(size_t)c2]);
  std::memcpy(sm + o_crow, crow.data(), (size_t)n_idx * sizeof(uint32_t));
  for (uint32_t idx = 0; idx < n_idx; idx++) { sm[o_info + 2 * idx] = 0u; sm[o_info + 2 * idx + 1] = 0xFFFFFFFFu; }      // the current tree, the home slots
  for (uint32_t c = 0; c < (uint32_t)pass.size(); c++) {
    sm[o_cost + 1 + c] = pass[c] ? 0u : 1u;
    sm[o_info + 2 * (1 + c)] = crow[1 + c];
    sm[o_info + 2 * (1 + c) + 1] = part[1 + c];
  }
  if (sel_rows) std::memcpy(sm + o_sel, sel_rows->data(), sel_rows->size() * sizeof(uint32_t));
  UCHK(hipMemcpyAsync(u.thr.p, sm, (o_cnt + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
  if (!have_C) { int rc = product(rows_p, sel_rows ? u.thr.p + o_sel : nullptr); if (rc) return rc; }
  uint32_t n_ev = 0;
  // the list rules and -storetrees see every (candidate, sample) at or below the sample's bound at the start of the step, not only the
  // strict improvements of a running minimum (as spr_sweeps_ufboot asks for them)
  const UfbExtract x{reinterpret_cast<const uint2 *>(u.thr.p + o_info), u.thr.p + o_cost, u.thr.p, u.thr.p + o_home, u.thr.p + o_crow, u.thr.p + o_best,
                     u.thr.p + o_cnt, n_idx, (u.topboot || u.distinct || u.store_trees) ? 1 : 0,
                     false};        // (no eager prefix: a step's events are fetched in one copy behind the count, as they always were here)
  { int rc = ufb_extract_events(x, n_ev); if (rc) return rc; }
  events.clear();
  if (n_ev) {
    events.assign(u.h_ev.p, u.h_ev.p + n_ev);
    for (UfbEvent &e : events) e.b = (uint32_t)u.ids[(size_t)e.b];
    if (!u.exchange) {                             // (a sample-sharded tracker orders the merged events: nni_exchange_events)
      std::vector<UfbEvent> tmp;
      std::vector<uint32_t> count;
      sort_events(events, tmp, count, n_idx, (uint32_t)u.B);
    }
  }
  u.events += n_ev;
  return MPF_OK;
}

// ---- one prune-node visit of a tracked climb ---------------------------------------------------------------------------------
// What a visit books around the two rules of spr_rule.hpp, in the reference's order: the current tree first (saveCurrentTree in
// front of the insertion tests, sprparsimony.cpp:2285-2289), every candidate before the tie rule sees it (:2163-2166), the
// cut-off test or the ratchet gate and the stale length with each booking, the pending trees or the log closed behind the scan,
// then the sweep's accept rule.  Every draw comes from one stream, so this order IS the behaviour.
// The three tracked loops fill in this state per batch and derive from it what differs between them:
//   bool next(const ScanPlan &, Cursor &, Cand &)        the visit's insertion tests in the reference's order
//   uint32_t stale_len(uint32_t idx, uint32_t home)      ratchet: a booked candidate's length on the original alignment
//   bool name_move(const ScanPlan &, long sel)           the selected move's records into insert_rec_ / remove_rec_
struct Engine::UfbVisit {
  struct Cand { size_t c; uint32_t idx, mp, home; };     // its number in the visit, output index, length, home index of its part
  struct Cursor { int pi = 0, k = 0; size_t c = 0; };    // where next() stands in the visit (a local of the replay: it stays in registers)
  Engine *e = nullptr;
  // the batch: the scan's costs, the events in replay order and how far they have been read
  const uint32_t *out = nullptr;
  const std::vector<UfbEvent> *events = nullptr;
  size_t ep = 0;
  // what is booked: the cut-off (host/ufb_cutoff.hpp), the ratchet gate (product_*: the batch has the REPS it reads), -storetrees
  bool ratchet = false, store_trees = false, product_self = true, product_cand = true;
  UfbCutoff cut;
  // the update rule: deferred (acceptances go to the log) or in place; the current tree's bookings from R_T on the host (h_rt) or
  // from events; self_row: the current tree has a cost and a product row of its own at every visit (asymmetric cost matrix)
  bool defer = false, host_self = true, self_row = false;
  const int32_t *h_rt = nullptr;
  bool *log_open = nullptr;
  SelfMoot *moot = nullptr;
  // a pipelined climb: worker_books = its log goes to a worker thread (option ufb_thread), which then owns refs, boot_trees, store
  // and topo_index; draws = its own counter, with or without that thread (null: UfbState::draws)
  bool worker_books = false;
  uint64_t *draws = nullptr;
  int32_t cur_plan = 0;
  // the visit's outcome
  long sel = -1;
  uint32_t sel_idx = 0, sel_home = 0;
  bool accept = false;
  std::vector<int32_t> mh_bk;                      // a candidate's topology and its canonical form
  std::string mh_key;

  uint32_t stale_len(uint32_t, uint32_t) const { return 0; }
  bool name_move(const ScanPlan &pl, long s)
  {
    e->insert_rec_ = e->candidate_record(pl, (size_t)s);
    e->remove_rec_ = s < pl.n_p ? pl.rec : e->back_[pl.rec];
    return true;
  }
};

// the insertion tests of a device-walked plan: part after part, idx = part_off + k, mp = base + out[idx], home = part_off + part_cnt
struct Engine::UfbPartsVisit : Engine::UfbVisit {
  // under a plain cut-off most insertion tests change nothing: not booked (above the cut-off) and longer than the best tree so far
  // (no counter, no draw) -- on to the next one that is either (best_ only falls while the block is read)
  bool skip_ahead = false;
  bool next(const ScanPlan &pl, Cursor &at, Cand &cd) const
  {
    for (; at.pi < pl.n_parts; at.pi++, at.k = 0) {
      const int cnt = pl.part_cnt[at.pi];
      if (skip_ahead && at.k < cnt) {
        const uint32_t lim_len = std::max(cut.none_pass ? 0u : cut.mp_max, e->best_);
        const int k2 = lim_len >= pl.base ? first_le(out + pl.part_off[at.pi], at.k, cnt, lim_len - pl.base) : cnt;
        at.c += (size_t)(k2 - at.k);
        at.k = k2;
      }
      if (at.k < cnt) {
        const uint32_t idx = pl.part_off[at.pi] + (uint32_t)at.k++;
        cd = Cand{at.c++, idx, pl.base + out[idx], pl.part_off[at.pi] + (uint32_t)cnt};
        return true;
      }
    }
    return false;
  }
};

template <class Loop>
int Engine::ufb_replay_visit(const ScanPlan &pl, Loop &L, uint32_t randomMP, unsigned &iter_hits)
{
  UfbState &u = *ufb_;
  if (tie_mode_ == MPF_TIE_RANDOM) {
    insert_rec_ = remove_rec_ = -1;
    hits_ = 1;
  }
  L.sel = -1;
  L.accept = false;
  auto draw = [&] { return tie_draw(); };
  // treels.find(tree_str) / treels[tree_str] = tree_index (iqtree.cpp:3500-3514, :3689-3707): a topology that some sample
  // accepted before keeps the index of that first tree
  auto topology_key = [&](uint32_t cand_code) -> const std::string & {
    if (cand_code == 0xFFFFFFFFu) {
      if (u.self_key_epoch != (uint64_t)topo_epoch_) { canonical_topology(back_, u.self_key); u.self_key_epoch = (uint64_t)topo_epoch_; }
      return u.self_key;
    }
    ufb_candidate_topology(cand_code < (uint32_t)pl.n_p ? pl.rec : back_[pl.rec], candidate_record(pl, (size_t)cand_code), L.mh_bk);
    canonical_topology(L.mh_bk, L.mh_key);
    return L.mh_key;
  };
  auto lookup_topology = [&](int64_t tree_index, uint32_t cand_code) -> int64_t {
    const double tl = now_ms();
    const int64_t ti = u.topo_index.emplace(topology_key(cand_code), tree_index).first->second;
    u.t_lookup += now_ms() - tl;
    u.lookups++;
    return ti;
  };
  uint64_t *draws = L.draws ? L.draws : &u.draws;
  const UfbDeferCtx dctx{L.defer, L.cur_plan, L.log_open, L.moot, draws};
  // the update rule of one booked tree over the samples whose events name output index idx
  auto replay_events = [&](uint32_t idx, int64_t tree_index, uint32_t cand_code) {
    const std::vector<UfbEvent> &ev = *L.events;
    while (L.ep < ev.size() && ev[L.ep].idx < idx) L.ep++;
    bool looked_up = L.store_trees;                // (-storetrees: tree_str is set at the top, no lookup per sample)
    for (; L.ep < ev.size() && ev[L.ep].idx == idx; L.ep++) ufb_one_event(ev[L.ep].b, ev[L.ep].s, tree_index, looked_up, cand_code, lookup_topology, dctx);
  };
  // one tree of length len arriving at saveCurrentTree.  A re-weighted (ratchet) climb is filtered by the length booked last
  // (iqtree.cpp:3283-3295 then :3343): a tree that fails leaves _pattern_pars as it is, so every later tree of the climb fails too
  // (-storetrees: unless a known topology gets in past the cut-off)
  // (copies: the bookings below write through pointers the compiler cannot tell from L's fields)
  const bool ratchet = L.ratchet, store_trees = L.store_trees, grow_refs = !L.worker_books;
  const UfbCutoff cut = L.cut;
  auto book = [&](uint32_t len, bool product, uint32_t cand_code) -> int64_t {
    bool pass;
    if (!ratchet) pass = cut.passes(len);
    else {
      pass = (store_trees || !u.gate_closed) && product && cut.passes(u.stale_len);
      if (!pass) u.gate_closed = true;
    }
    const uint32_t cur_len = ratchet ? u.stale_len : len;
    u.cur_logl_now = -(int32_t)cur_len;
    return ufb_book_tree(cur_len, pass, cand_code, store_trees, topology_key, grow_refs);
  };
  if (pl.self_idx >= 0) {
    // rearrangeParsimony's evaluateParsimony(p) + pllSaveCurrentTreeSprParsimony (sprparsimony.cpp:2285-2289): the current tree,
    // once per prune node and before any of its insertion tests
    const uint32_t self_idx = (uint32_t)pl.self_idx;
    int64_t tree_index = book(L.self_row ? L.out[self_idx] : randomMP, L.product_self, 0xFFFFFFFFu);
    if (tree_index >= 0) {
      // it scores R_T[b] for every sample: no device events for its slots where the host has R_T (they would be B per visit, 2.0e6
      // per move-less C3 sweep, all to be copied and ordered) -- the host offers it to every sample in order
      if (!L.host_self) replay_events(self_idx, tree_index, 0xFFFFFFFFu);
      else if (L.defer) ufb_self_default(L.h_rt, tree_index, L.cur_plan, *L.log_open, *draws, L.moot);
      else {
        bool looked_up = L.store_trees;
        for (int c2 = 0; c2 < u.Bl; c2++) ufb_one_event((uint32_t)u.ids[(size_t)c2], (uint32_t)L.h_rt[c2], tree_index, looked_up, 0xFFFFFFFFu, lookup_topology, dctx);
      }
      if (L.ratchet) u.stale_len = L.self_row ? L.stale_len(self_idx, self_idx) : u.rt_orig;     // _pattern_pars now holds the current tree
    }
  }
  const bool product_cand = L.product_cand;
  typename Loop::Cursor at;
  typename Loop::Cand cd, taken{0, 0, 0, 0};
  long sel = -1;
  while (L.next(pl, at, cd)) {
    const int64_t tree_index = book(cd.mp, product_cand, (uint32_t)cd.c);        // saveCurrentTree(-mp), sprparsimony.cpp:2163-2166
    if (tree_index >= 0) {
      replay_events(cd.idx, tree_index, (uint32_t)cd.c);
      // pllComputePatternParsimony (iqtree.cpp:3365) has now refreshed _pattern_pars for THIS candidate: its length on the
      // original alignment is what the next call will see
      if (ratchet) u.stale_len = L.stale_len(cd.idx, cd.home);
    }
    if (sprrule::offer(tie_mode_, cd.mp, best_, hits_, draw)) { sel = (long)cd.c; taken = cd; }
  }
  L.sel = sel; L.sel_idx = taken.idx; L.sel_home = taken.home;
  if (L.sel >= 0 && !L.name_move(pl, L.sel)) return MPF_E_STATE;
  // topologies of the trees accepted during this scan that some sample still points to, or the end-of-prune-node mark of the log
  if (!L.defer) ufb_flush_pending(pl);
  else if (*L.log_open) { u.log.push_back(UfbState::LogEntry{0xFFFFFFFFu, 0u, 0, L.cur_plan}); *L.log_open = false; }
  L.accept = sprrule::accept(tie_mode_, best_, randomMP, iter_hits, remove_rec_ >= 0 && insert_rec_ >= 0, draw);
  if (L.accept && L.sel < 0) { set_error("online UFBoot: accepted move without a candidate of this prune node"); return MPF_E_STATE; }
  return MPF_OK;
}

// ---- the batch scaffolding of the tracked loops ------------------------------------------------------------------------------
// the first prune node of a batch with a strictly better candidate than the current tree ends the batch for certain (a tie may end
// it earlier): its number, or np - 1
static inline int ufb_first_better(const std::vector<ScanPlan> &plans, int np, const uint32_t *out, uint32_t randomMP)
{
  for (int j = 0; j < np; j++) {
    const ScanPlan &pl = plans[(size_t)j];
    uint32_t m = UINT32_MAX;
    for (int pi = 0; pi < pl.n_parts; pi++)
      for (int k = 0; k < pl.part_cnt[pi]; k++) m = std::min(m, out[pl.part_off[pi] + (uint32_t)k]);
    if (m != UINT32_MAX && pl.base + m < randomMP) return j;
  }
  return np - 1;
}

// what lies behind that prune node is never replayed: one past the last output index in front of it (n_idx: the whole batch)
static inline uint32_t ufb_index_cut(const std::vector<ScanPlan> &plans, int np, const uint32_t *out, uint32_t randomMP, uint32_t n_idx)
{
  const int js = ufb_first_better(plans, np, out, randomMP);
  if (js == np - 1) return n_idx;
  uint32_t cut = 0;
  for (int j = 0; j <= js; j++) {
    const ScanPlan &pl = plans[(size_t)j];
    if (pl.self_idx >= 0) cut = std::max(cut, (uint32_t)pl.self_idx + 1u);
    for (int pi = 0; pi < pl.n_parts; pi++) cut = std::max(cut, pl.part_off[pi] + (uint32_t)pl.part_cnt[pi] + 1u);
  }
  return cut;
}

}  // namespace mpf
