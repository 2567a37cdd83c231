// refresh_plan_main.cpp -- the host-only planner of the view refresh (refresh_plan.hpp) as a stand-alone program: no device, no
// engine, nothing loaded into another process.  tests/test_refresh_plan_host.py builds it with -fsanitize=address,undefined and
// feeds it seeded cases; every plan is checked by executing it, not by comparing it with another planner.
//
//   refresh_plan FILE    FILE: binary int32, any number of cases
//                        n, start, n_roots (-1: the whole tree), n_list (-1: the topology array is rebuilt wholesale),
//                        back[R], valid[R], roots[n_roots], list[n_list], and if n_list >= 0 the links before the edit: old[R]
//                        (R = 3 (2n - 1) + 3 records, as the engine keeps them)
//   Prints one line per case: ops, levels, chain levels, the largest number of chains in one level.  A plan that fails a check
//   is reported on stderr and ends the run with status 1.
//
// The execution: every tip holds a distinct 64-bit value, vec[r] = mix(vec[back[nx r]], vec[back[nx nx r]]) with a mix that does
// not commute.  Vectors valid on entry hold what the plain recursion over back gives; an op may read tips, those, and results of
// strictly earlier levels.  Afterwards every requested root holds the recursion's value.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <string>

#include "refresh_plan.hpp"

using namespace mpf;

static int g_case = 0;
#define CHECK(cond, ...)                                                                \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      std::fprintf(stderr, "case %d: %s: ", g_case, #cond);                             \
      std::fprintf(stderr, __VA_ARGS__);                                                \
      std::fprintf(stderr, "\n");                                                       \
      std::exit(1);                                                                     \
    }                                                                                   \
  } while (0)

static uint64_t mix(uint64_t a, uint64_t b) { return (a * 0x9E3779B97F4A7C15ull + ((b << 23) | (b >> 41))) ^ 0xD1B54A32D192ED03ull; }
static uint64_t tip_value(int t) { uint64_t z = (uint64_t)t * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull; return z ^ (z >> 29); }

struct Case {
  int n = 0, start = 0, R = 0;
  std::vector<int32_t> back, old;
  std::vector<uint8_t> valid;
  std::vector<int> roots, list;
  bool full = false, wholesale = false;
  uint32_t slot(int r) const { const int v = r / 3; return v <= n ? (uint32_t)(v - 1) : (uint32_t)(n + 3 * (v - n - 1) + r % 3); }
  size_t nslots() const { return (size_t)n + 3 * ((size_t)n - 2); }
  bool tip(int r) const { return r / 3 <= n; }
};
static int nx(int r) { return RefreshPlanner::nx(r); }

// the state of the simulated vector store
struct Store {
  std::vector<uint64_t> val, truth;
  std::vector<int> level;                        // 0: readable on entry (tip or valid), > 0: written at that level, -1: stale
  std::vector<int> rec_of;                       // slot -> record
};

static Store fresh_store(const Case &c)
{
  Store s;
  s.val.assign(c.nslots(), 0xDEADDEADDEADDEADull);
  s.truth.assign(c.nslots(), 0);
  s.level.assign(c.nslots(), -1);
  s.rec_of.assign(c.nslots(), -1);
  std::vector<char> known(c.nslots(), 0);
  std::function<uint64_t(int)> value = [&](int r) -> uint64_t {
    if (c.tip(r)) return tip_value(r / 3);
    const uint32_t sl = c.slot(r);
    if (!known[sl]) {
      s.truth[sl] = mix(value(c.back[(size_t)nx(r)]), value(c.back[(size_t)nx(nx(r))]));
      known[sl] = 1;
    }
    return s.truth[sl];
  };
  for (int t = 1; t <= c.n; t++) { s.val[(size_t)t - 1] = s.truth[(size_t)t - 1] = tip_value(t); s.level[(size_t)t - 1] = 0; s.rec_of[(size_t)t - 1] = 3 * t; }
  for (int r = 3 * (c.n + 1); r < 3 * (2 * c.n - 1); r++) {
    if (c.back[(size_t)r] < 0) continue;
    const uint32_t sl = c.slot(r);
    s.rec_of[sl] = r;
    value(r);
    if (c.valid[(size_t)r]) { s.val[sl] = s.truth[sl]; s.level[sl] = 0; }
  }
  return s;
}

static uint64_t read_mem(const Store &s, uint32_t sl, int level, const char *what)
{
  CHECK(sl < s.level.size(), "%s: slot %u out of range", what, sl);
  CHECK(s.level[sl] >= 0 && s.level[sl] < level, "%s: slot %u read at level %d, written at %d", what, sl, level, s.level[sl]);
  return s.val[sl];
}

static void write_mem(const Case &c, Store &s, const PlanOp &o, uint64_t v, int level)
{
  const int r = (int)o.pad;
  CHECK(r >= 3 * (c.n + 1) && r < 3 * (2 * c.n - 1) && c.slot(r) == o.dst, "op of record %d writes slot %u", r, o.dst);
  CHECK(!c.valid[(size_t)r], "record %d was valid on entry", r);
  CHECK(s.level[o.dst] == -1, "slot %u written twice", o.dst);
  s.val[o.dst] = v;
  s.level[o.dst] = level;
}

static void check_result(const Case &c, const Store &s, const std::vector<int> &roots, size_t nops, const std::vector<int> &upd, const std::vector<PlanOp> &ops)
{
  size_t written = 0;
  for (size_t sl = 0; sl < s.level.size(); sl++) {
    if (s.level[sl] > 0) written++;
    if (s.level[sl] >= 0) CHECK(s.val[sl] == s.truth[sl], "slot %zu holds a wrong value", sl);
  }
  CHECK(written == nops, "%zu slots written by %zu ops", written, nops);
  for (int r : roots)
    if (r >= 0 && !c.tip(r)) CHECK(s.level[c.slot(r)] >= 0, "root %d left stale", r);
  CHECK(upd.size() == nops, "upd_order has %zu entries", upd.size());
  for (size_t i = 0; i < nops; i++) CHECK(upd[i] == (int)ops[i].pad, "upd_order[%zu]", i);
}

static void run_case(const Case &c, RefreshPlanner &pl)
{
  const auto slot_of = [&](int r) { return c.slot(r); };
  for (int r = 3 * (c.n + 1); r < 3 * (2 * c.n - 1); r++) {     // the engine's invariant, so that the case itself is sound
    if (!c.valid[(size_t)r]) continue;
    for (int in : {c.back[(size_t)nx(r)], c.back[(size_t)nx(nx(r))]}) CHECK(c.tip(in) || c.valid[(size_t)in], "valid record %d has a stale input", r);
  }
  pl.bind(c.n, c.back.data(), c.valid.data(), (size_t)c.R);
  std::vector<int> roots = c.roots;
  if (c.full) { pl.whole_tree(c.start); roots = pl.all; CHECK(roots.size() == 3 * ((size_t)c.n - 2), "whole_tree lists %zu records", roots.size()); }
  bool none_valid = true;
  for (uint8_t v : c.valid) none_valid = none_valid && !v;
  const bool from_scratch = c.full && none_valid;
  pl.close(roots, from_scratch);
  const std::vector<int> order = pl.order;
  const size_t nops = order.size();
  const int maxlev = pl.maxlev;
  std::vector<int> lev_of((size_t)c.R, 0);
  for (int r : order) lev_of[(size_t)r] = pl.lev[(size_t)r];
  if (from_scratch) {
    // the two-sweep shortcut and the generic closure: the same ops, the same level per op
    CHECK(nops == 3 * ((size_t)c.n - 2), "from scratch: %zu ops", nops);
    pl.close(roots, false);
    CHECK(pl.order.size() == nops && pl.maxlev == maxlev, "generic closure: %zu ops, %d levels", pl.order.size(), pl.maxlev);
    for (int r : pl.order) CHECK(pl.lev[(size_t)r] == lev_of[(size_t)r], "record %d: level %d vs %d", r, pl.lev[(size_t)r], lev_of[(size_t)r]);
    pl.close(roots, true);
  }
  // ---- the topology array: deltas against a full rebuild
  {
    std::vector<uint32_t> want(2 * c.nslots(), 0), kids(2 * c.nslots(), 0), applied;
    auto rebuild = [&](const std::vector<int32_t> &back, std::vector<uint32_t> &k) {
      for (int r = 3 * (c.n + 1); r < 3 * (2 * c.n - 1); r++) {
        k[2 * (size_t)c.slot(r)] = c.slot(back[(size_t)nx(r)]);
        k[2 * (size_t)c.slot(r) + 1] = c.slot(back[(size_t)nx(nx(r))]);
      }
    };
    rebuild(c.back, want);
    if (!c.wholesale) rebuild(c.old, kids);
    applied = kids;
    const bool changed = pl.topo_delta(kids.data(), c.list, c.wholesale, roots, c.full, true, slot_of);
    CHECK(changed == (!c.wholesale && !c.list.empty()), "topo_delta's answer");
    CHECK(pl.kid_upd.size() % 3 == 0, "kid_upd has %zu words", pl.kid_upd.size());
    for (size_t i = 0; i < pl.kid_upd.size(); i += 3) {
      CHECK(pl.kid_upd[i] >= (uint32_t)c.n && pl.kid_upd[i] < c.nslots(), "kid_upd slot %u", pl.kid_upd[i]);
      applied[2 * (size_t)pl.kid_upd[i]] = pl.kid_upd[i + 1];
      applied[2 * (size_t)pl.kid_upd[i] + 1] = pl.kid_upd[i + 2];
    }
    CHECK(applied == kids, "the triples and the mirror disagree");
    // a wholesale rebuild covers what the refresh touches: the roots and every op
    for (size_t sl = c.n; sl < c.nslots(); sl++) {
      const int r = 3 * (c.n + 1) + (int)(sl - (size_t)c.n);
      const bool covered = !c.wholesale || c.full || lev_of[(size_t)r] > 0;
      if (covered) CHECK(kids[2 * sl] == want[2 * sl] && kids[2 * sl + 1] == want[2 * sl + 1], "kids of slot %zu", sl);
    }
    pl.topo_delta(kids.data(), c.list, c.wholesale, roots, c.full, false, slot_of);
    CHECK(pl.kid_upd.empty(), "triples emitted unasked");
  }
  // ---- level form
  std::vector<PlanOp> ops(nops + 1);
  std::vector<int32_t> lo((size_t)maxlev + 2, -1);
  std::vector<int> upd;
  if (nops) {
    pl.emit_levels(ops.data(), lo.data(), upd, slot_of);
    Store s = fresh_store(c);
    CHECK(lo[0] == 0 && lo[(size_t)maxlev] == (int32_t)nops, "level offsets run from %d to %d", lo[0], lo[(size_t)maxlev]);
    for (int l = 1; l <= maxlev; l++) {
      CHECK(lo[(size_t)l - 1] < lo[(size_t)l], "level %d is empty", l);
      for (int i = lo[(size_t)l - 1]; i < lo[(size_t)l]; i++) {
        const PlanOp &o = ops[(size_t)i];
        CHECK(lev_of[o.pad < (uint32_t)c.R ? o.pad : 0] == l, "op %d sits in level %d", i, l);
        write_mem(c, s, o, mix(read_mem(s, o.a, l, "a"), read_mem(s, o.b, l, "b")), l);
      }
    }
    check_result(c, s, roots, nops, upd, ops);
  } else {
    for (int r : roots) CHECK(r < 0 || c.tip(r) || c.valid[(size_t)r], "no ops, but root %d is stale", r);
  }
  // ---- chain form: per (level, wave) range of ch_off a link continues the op before it
  int max_chains = 0;
  if (nops) {
    pl.build_chains();
    std::vector<int32_t> off(pl.ch_off.size(), -1);
    pl.emit_chains(ops.data(), off.data(), upd, slot_of);
    Store s = fresh_store(c);
    CHECK(off.size() == (size_t)pl.ch_levels * 16 + 1 && off[0] == 0 && off.back() == (int32_t)nops, "chain offsets");
    for (int l = 0; l < pl.ch_levels; l++) {
      int chains = 0;
      std::vector<std::pair<PlanOp, uint64_t>> out;
      for (int w = 0; w < 16; w++) {
        const int b = off[(size_t)l * 16 + (size_t)w], e = off[(size_t)l * 16 + (size_t)w + 1];
        CHECK(b <= e, "chain offsets go down at level %d wave %d", l, w);
        uint64_t reg = 0;
        for (int i = b; i < e; i++) {
          const PlanOp &o = ops[(size_t)i];
          const int r = (int)o.pad;
          CHECK(r >= 3 * (c.n + 1) && r < 3 * (2 * c.n - 1), "op %d: record %d", i, r);
          const uint32_t in0 = c.slot(c.back[(size_t)nx(r)]), in1 = c.slot(c.back[(size_t)nx(nx(r))]);
          uint64_t v;
          if (o.a != 0xFFFFFFFFu) {                // a head: both operands from memory
            chains++;
            v = mix(read_mem(s, o.a, l + 1, "head a"), read_mem(s, o.b, l + 1, "head b"));
          } else {
            CHECK(i > b, "a link opens the range of level %d wave %d", l, w);
            const uint32_t prev = ops[(size_t)i - 1].dst;
            CHECK((prev == in0 && o.b == in1) || (prev == in1 && o.b == in0), "link %d: previous result %u, other %u, inputs %u %u", i, prev, o.b, in0, in1);
            const uint64_t m = read_mem(s, o.b, l + 1, "link");
            v = prev == in0 ? mix(reg, m) : mix(m, reg);
          }
          reg = v;
          out.emplace_back(o, v);
        }
      }
      // results reach memory when the level is done: nothing of this level was read from memory within it
      for (auto &p : out) write_mem(c, s, p.first, p.second, l + 1);
      max_chains = std::max(max_chains, chains);
    }
    check_result(c, s, roots, nops, upd, ops);
  }
  std::printf("case %d ops %zu levels %d chain_levels %d max_chains %d\n", g_case, nops, maxlev, nops ? pl.ch_levels : 0, max_chains);
}

int main(int argc, char **argv)
{
  if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  RefreshPlanner pl;                               // one planner for every case, as the engine keeps one: scratch carries over
  int32_t head[4];
  while (in.read(reinterpret_cast<char *>(head), sizeof(head))) {
    Case c;
    c.n = head[0];
    c.start = head[1];
    if (c.n < 4 || c.n > 100000) { std::fprintf(stderr, "bad header\n"); return 2; }
    c.R = 3 * (2 * c.n - 1) + 3;
    c.full = head[2] < 0;
    c.wholesale = head[3] < 0;
    auto read_ints = [&](size_t k) {
      std::vector<int32_t> v(k);
      in.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(k * sizeof(int32_t)));
      return v;
    };
    c.back = read_ints((size_t)c.R);
    const std::vector<int32_t> valid = read_ints((size_t)c.R);
    c.valid.assign(valid.begin(), valid.end());
    const std::vector<int32_t> roots = read_ints(c.full ? 0 : (size_t)head[2]), list = read_ints(c.wholesale ? 0 : (size_t)head[3]);
    c.roots.assign(roots.begin(), roots.end());
    c.list.assign(list.begin(), list.end());
    if (!c.wholesale) c.old = read_ints((size_t)c.R);
    if (!in) { std::fprintf(stderr, "short file\n"); return 2; }
    run_case(c, pl);
    g_case++;
  }
  return 0;
}
