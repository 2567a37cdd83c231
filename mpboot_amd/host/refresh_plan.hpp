// refresh_plan.hpp -- the host-only part of the view refresh (Engine::schedule_views*): which directional vectors a refresh
// recomputes and in what order, and where the pieces of its upload lie.  No device code, no engine, so that it can be compiled
// into a stand-alone program and run under a sanitizer (host/refresh_plan_main.cpp, tests/test_refresh_plan_host.py).
//
// Records as everywhere: rec = 3 * node + slot, tips are nodes 1 .. n, vec[r] (r inner) = f(vec[back[nx r]], vec[back[nx nx r]]).
// RefreshStage: the byte layout of the staging buffer, [kids][prune records][ops][level offsets][level count][deltas][rides].
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace mpf {

struct PlanOp { uint32_t dst, a, b, pad; };      // NvOp's layout (kernels.hpp; engine.cpp asserts it)
struct RefreshStage { size_t kids_bytes, nodep_off, ops_off, lev_off, nlev_off, upd_off, ride_off[2], total; };

// Every region starts on a 16-byte boundary.  The host's schedule has no prune records (nodep_off == ops_off) and no level count
// (count_bytes 0: upd_off == nlev_off); the device's has no deltas and no rides.  ride_off[i] == 0: nothing rides.
inline RefreshStage refresh_stage(size_t nslots, size_t nops, size_t n_offsets, size_t n_prune, size_t count_bytes, size_t upd_words,
                                  const size_t ride_bytes[2])
{
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  RefreshStage s;
  s.kids_bytes = nslots * 8;
  s.nodep_off = up(s.kids_bytes);
  s.ops_off = s.nodep_off + up(n_prune * sizeof(uint32_t));
  s.lev_off = s.ops_off + up(nops * sizeof(PlanOp));
  s.nlev_off = s.lev_off + up(n_offsets * sizeof(int32_t));
  s.upd_off = s.nlev_off + count_bytes;
  s.total = s.upd_off + up(upd_words * sizeof(uint32_t));
  for (int i = 0; i < 2; i++) {
    s.ride_off[i] = ride_bytes[i] ? s.total : 0;
    s.total += up(ride_bytes[i]);
  }
  return s;
}

// Scratch lives in members: a refresh is planned once per scan batch of a climb, allocations would show.
struct RefreshPlanner {
  int n = 0;
  const int32_t *back = nullptr;
  const uint8_t *valid = nullptr;
  std::vector<int> all, stack, order;
  std::vector<int32_t> lev, lev_epoch, ch_off;    // ch_off: first op of every (level, wave), 16 waves per level
  std::vector<uint32_t> kid_upd;
  int32_t epoch = 0;
  int maxlev = 0, ch_levels = 0;

  // the tree's arrays, nrec records each: they stay the caller's, who edits them between the calls below
  void bind(int n_, const int32_t *back_, const uint8_t *valid_, size_t nrec) { n = n_; back = back_; valid = valid_; lev.assign(nrec, 0); lev_epoch.assign(nrec, 0); }
  bool tip(int r) const { return r / 3 <= n; }
  static int nx(int r) { const int v = r / 3, s = r % 3; return 3 * v + (s + 1) % 3; }

  void whole_tree(int start)
  {
    all.clear();
    stack.clear();
    seen_.assign(2 * (size_t)n + 1, 0);
    stack.push_back(back[start]);
    while (!stack.empty()) {
      const int r = stack.back();                  // the record by which the node is entered: it faces the root (start)
      stack.pop_back();
      if (r < 0 || tip(r) || seen_[(size_t)(r / 3)]) continue;
      seen_[(size_t)(r / 3)] = 1;
      all.push_back(r);
      all.push_back(nx(r));
      all.push_back(nx(nx(r)));
      stack.push_back(back[nx(nx(r))]);
      stack.push_back(back[nx(r)]);
    }
  }

  // from_scratch: roots is `all` (whole_tree) and nothing is valid
  void close(const std::vector<int> &roots, bool from_scratch)
  {
    epoch++;
    order.clear();
    pairs_.clear();
    auto lev_of = [&](int r) { return (tip(r) || lev_epoch[r] != epoch) ? 0 : lev[r]; };
    if (from_scratch) {
      // two sweeps over the tree rooted at start instead of the generic closure
      // views looking away from the root, children first: level = height
      for (size_t i = all.size(); i >= 3; i -= 3) {
        const int u = all[i - 3];
        const int a = back[nx(u)], b = back[nx(nx(u))];
        lev[u] = 1 + std::max(tip(a) ? 0 : lev[a], tip(b) ? 0 : lev[b]);
        lev_epoch[u] = epoch;
        order.push_back(u);
      }
      // views looking towards the root, parents first: inputs are the parent's view towards us and the sibling's subtree
      for (size_t i = 0; i < all.size(); i += 3) {
        const int u = all[i], r1 = nx(u), r2 = nx(r1);
        const int p = back[u], c1 = back[r1], c2 = back[r2];
        const int lp = tip(p) ? 0 : lev[p];
        lev[r1] = 1 + std::max(lp, tip(c2) ? 0 : lev[c2]);
        lev[r2] = 1 + std::max(lp, tip(c1) ? 0 : lev[c1]);
        lev_epoch[r1] = lev_epoch[r2] = epoch;
        order.push_back(r1);
        order.push_back(r2);
      }
    }
    for (int r0 : roots) {
      if (from_scratch) break;
      if (r0 < 0 || tip(r0) || valid[r0] || lev_epoch[r0] == epoch) continue;
      pairs_.emplace_back(r0, 0);
      while (!pairs_.empty()) {
        auto &top = pairs_.back();
        const int r = top.first;
        const int a = back[nx(r)], b = back[nx(nx(r))];
        if (top.second == 0) {
          top.second = 1;
          if (!tip(a) && !valid[a] && lev_epoch[a] != epoch) { pairs_.emplace_back(a, 0); continue; }
        }
        if (top.second == 1) {
          top.second = 2;
          if (!tip(b) && !valid[b] && lev_epoch[b] != epoch) { pairs_.emplace_back(b, 0); continue; }
        }
        if (lev_epoch[r] != epoch) {
          lev[r] = 1 + std::max(lev_of(a), lev_of(b));
          lev_epoch[r] = epoch;
          order.push_back(r);
        }
        pairs_.pop_back();
      }
    }
    maxlev = 0;
    for (int r : order) maxlev = std::max(maxlev, lev[r]);
  }

  // ops[] in level order; lo[l] = first op of level l + 1, lo[maxlev] = the number of ops (maxlev + 2 entries are written);
  // upd_order: the records in the order of their ops
  template <class Op, class Slot>
  void emit_levels(Op *ops, int32_t *lo, std::vector<int> &upd_order, Slot slot)
  {
    const size_t nops = order.size();
    for (int l = 0; l <= maxlev + 1; l++) lo[l] = 0;
    for (int r : order) lo[lev[r]]++;
    int acc = 0;
    for (int l = 1; l <= maxlev; l++) { const int c = lo[l]; lo[l] = acc; acc += c; }
    lo[0] = 0;
    fill_.assign(lo, lo + maxlev + 1);
    upd_order.resize(nops);
    for (int r : order) {
      const int at = fill_[lev[r]]++;
      Op &o = ops[at];
      o.dst = slot(r);
      o.a = slot(back[nx(r)]);
      o.b = slot(back[nx(nx(r))]);
      o.pad = (uint32_t)r;
      upd_order[(size_t)at] = r;
    }
    for (int l = 1; l <= maxlev; l++) lo[l - 1] = lo[l];
    lo[maxlev] = (int32_t)nops;
  }

  // Brings kids[] (two words per slot) up to date: `dirty` = wholesale (every root and, unless the roots hold every op, every op),
  // else the records of kids_list.  emit: the changes also go to kid_upd as (slot, kid, kid) for a kernel to apply.
  // Returns whether the listed records changed anything in kids[].
  template <class Slot>
  bool topo_delta(uint32_t *kids, const std::vector<int> &kids_list, bool dirty, const std::vector<int> &roots, bool full, bool emit, Slot slot)
  {
    kid_upd.clear();
    auto put = [&](int r) {
      const uint32_t s = slot(r), x = slot(back[nx(r)]), y = slot(back[nx(nx(r))]);
      kids[2 * (size_t)s] = x;
      kids[2 * (size_t)s + 1] = y;
      if (emit) { kid_upd.push_back(s); kid_upd.push_back(x); kid_upd.push_back(y); }
    };
    if (!dirty) {
      for (int r : kids_list)
        if (back[r] >= 0) put(r);
      return !kids_list.empty();
    }
    for (int r : roots)
      if (r >= 0 && !tip(r)) put(r);
    if (!full)
      for (int r : order) put(r);
    return false;
  }

  // Cut the refresh's dependency graph (ops = `order`, topologically sorted) into chains for k_newview_chain: op j continues
  // the chain of op d when d is j's ONLY stale input (its other input is valid already, so the wave can prefetch it); of the
  // up to two consumers of d the one with the longer path above it continues, the other starts a chain of the next level.
  // A chain's level is one more than the deepest chain it takes an input from; per level the chains are spread over the 16
  // waves of a workgroup, longest first.  -> ch_off (first op of every level and wave), ch_levels; emit_chains writes the ops
  void build_chains()
  {
    const int N = (int)order.size();
    if (idx_.size() != lev.size()) idx_.assign(lev.size(), 0);
    for (int i = 0; i < N; i++) idx_[(size_t)order[(size_t)i]] = i;
    auto dep_of = [&](int x) { return (!tip(x) && lev_epoch[x] == epoch) ? idx_[(size_t)x] : -1; };
    d0_.resize((size_t)N); d1_.resize((size_t)N); h_.assign((size_t)N, 0); next_.assign((size_t)N, -1);
    chain_.resize((size_t)N);
    for (int i = 0; i < N; i++) {
      const int r = order[(size_t)i];
      d0_[(size_t)i] = dep_of(back[nx(r)]);
      d1_[(size_t)i] = dep_of(back[nx(nx(r))]);
    }
    for (int i = N - 1; i >= 0; i--) {
      const int h = h_[(size_t)i] + 1;
      const int d0 = d0_[(size_t)i], d1 = d1_[(size_t)i];
      if (d0 >= 0 && h_[(size_t)d0] < h) h_[(size_t)d0] = h;
      if (d1 >= 0 && h_[(size_t)d1] < h) h_[(size_t)d1] = h;
    }
    auto single = [&](int j) { const int d0 = d0_[(size_t)j], d1 = d1_[(size_t)j]; return (d0 >= 0) != (d1 >= 0) ? (d0 >= 0 ? d0 : d1) : -1; };
    for (int j = 0; j < N; j++) {
      const int d = single(j);
      if (d >= 0 && (next_[(size_t)d] < 0 || h_[(size_t)j] > h_[(size_t)next_[(size_t)d]])) next_[(size_t)d] = j;
    }
    // chains in order of their heads; level of a chain from its head's inputs
    head_.clear(); len_.clear(); slev_.clear();
    int nlev = 0;
    for (int j = 0; j < N; j++) {
      const int d = single(j);
      if (d >= 0 && next_[(size_t)d] == j) continue;            // a link, reached from its head
      const int c = (int)head_.size();
      int l = 0;
      if (d0_[(size_t)j] >= 0) l = std::max(l, slev_[(size_t)chain_[(size_t)d0_[(size_t)j]]] + 1);
      if (d1_[(size_t)j] >= 0) l = std::max(l, slev_[(size_t)chain_[(size_t)d1_[(size_t)j]]] + 1);
      int len = 0;
      for (int k = j; k >= 0; k = next_[(size_t)k]) { chain_[(size_t)k] = c; len++; }
      head_.push_back(j);
      len_.push_back(len);
      slev_.push_back(l);
      nlev = std::max(nlev, l + 1);
    }
    const int C = (int)head_.size();
    // per level: chains longest first onto the least loaded wave
    lev_off_.assign((size_t)nlev + 1, 0);
    for (int c = 0; c < C; c++) lev_off_[(size_t)slev_[(size_t)c] + 1]++;
    for (int l = 0; l < nlev; l++) lev_off_[(size_t)l + 1] += lev_off_[(size_t)l];
    sorted_.resize((size_t)C);
    fill_.assign(lev_off_.begin(), lev_off_.end() - 1);
    for (int c = 0; c < C; c++) sorted_[(size_t)fill_[(size_t)slev_[(size_t)c]]++] = c;
    wave_.resize((size_t)C);
    ch_off.assign((size_t)nlev * 16 + 1, 0);
    for (int l = 0; l < nlev; l++) {
      int *b = sorted_.data() + lev_off_[(size_t)l], *e = sorted_.data() + lev_off_[(size_t)l + 1];
      if (e - b > 16) std::sort(b, e, [&](int x, int y) { return len_[(size_t)x] != len_[(size_t)y] ? len_[(size_t)x] > len_[(size_t)y] : x < y; });
      int load[16] = {0};
      for (int *p = b; p < e; p++) {
        int w = 0;
        for (int k = 1; k < 16; k++) if (load[k] < load[w]) w = k;
        wave_[(size_t)*p] = w;
        load[w] += len_[(size_t)*p];
      }
      for (int w = 0; w < 16; w++) ch_off[(size_t)l * 16 + (size_t)w + 1] = load[w];
    }
    for (size_t i = 1; i < ch_off.size(); i++) ch_off[i] += ch_off[i - 1];
    ch_levels = nlev;
  }

  // the chains' ops where the caller says, per (level, wave) range of ch_off; off[] takes ch_off
  template <class Op, class Slot>
  void emit_chains(Op *ops, int32_t *off, std::vector<int> &upd_order, Slot slot)
  {
    upd_order.resize(order.size());
    fill_.assign(ch_off.begin(), ch_off.end() - 1);
    for (int l = 0; l < ch_levels; l++)
      for (int i = lev_off_[(size_t)l]; i < lev_off_[(size_t)l + 1]; i++) {
        const int c = sorted_[(size_t)i];
        int &at = fill_[(size_t)l * 16 + (size_t)wave_[(size_t)c]];
        for (int k = head_[(size_t)c]; k >= 0; k = next_[(size_t)k], at++) {
          const int r = order[(size_t)k];
          const bool head = k == head_[(size_t)c];
          Op &o = ops[at];
          o.dst = slot(r);
          o.a = head ? slot(back[nx(r)]) : 0xFFFFFFFFu;          // a link takes the previous result from registers ...
          // ... and from memory the input that is NOT the previous op
          o.b = slot(back[head || d0_[(size_t)k] >= 0 ? nx(nx(r)) : nx(r)]);
          o.pad = (uint32_t)r;
          upd_order[(size_t)at] = r;
        }
      }
    std::memcpy(off, ch_off.data(), ch_off.size() * sizeof(int32_t));
  }

 private:
  std::vector<int> fill_, idx_, d0_, d1_, h_, next_, chain_, head_, len_, slev_, lev_off_, sorted_, wave_;
  std::vector<char> seen_;
  std::vector<std::pair<int, int>> pairs_;
};

}  // namespace mpf
