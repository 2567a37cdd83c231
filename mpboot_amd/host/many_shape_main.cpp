// many_shape_main.cpp -- the shape rule of a round of mpf_optimize_spr_many_round (many_shape.hpp) as a stand-alone program: no
// device, no engine, nothing loaded into another process.  tests/test_many_shape_host.py builds it with
// -fsanitize=address,undefined and feeds it a table of cases.
//
//   many_shape FILE      FILE: text, one case per line: n, then per engine twelve integers
//                        state  now.vw now.S now.dev now.wm  pack_gen  fits  started.vw started.S started.dev started.wm  started_gen
//   Prints one line per case:
//     case I rc R vw V S S wm W dev D batch a,b,.. alone c,d,.. owner O | parent vw V batch a,b,.. foreign F [| MESSAGE]
//   (lists "-" when empty; owner -1 without a batch).  Behind the bar the rule this one replaced, "the shape of the first active
//   engine; only starting climbs are compared with it": the width it launches on, its batch, and how many CONTINUING climbs of
//   that batch were laid out for another width or word-major flag than the launch's -- climbs it would have run on foreign tiles.
//   Every plan of the rule in force is checked here: a batch member on another shape than the launch's, an active engine that is
//   neither in the batch nor alone, or one in both is reported on stderr and ends the run with status 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "many_shape.hpp"

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

// Engine::climb_many_round before the rule moved into many_shape.hpp
struct ParentPlan { int vw = 0; bool wm = false; std::vector<int> batch, alone; int foreign = 0; };
static ParentPlan parent_rule(const std::vector<ManyEntry> &e)
{
  ParentPlan p;
  int first = -1;
  for (size_t k = 0; k < e.size(); k++) if (e[k].state) { first = (int)k; break; }
  if (first < 0) return p;
  const ManyShape &s0 = e[(size_t)first].now;
  p.vw = s0.vw;
  p.wm = s0.wm;
  for (size_t k = 0; k < e.size(); k++) {
    if (e[k].state == 1) {
      const bool fits = s0.vw > 0 && e[k].fits && e[k].now.dev == s0.dev && e[k].now.S == s0.S && e[k].now.vw == s0.vw;
      (fits ? p.batch : p.alone).push_back((int)k);
    } else if (e[k].state == 2) {
      p.batch.push_back((int)k);                   // (never compared with anything)
      if (e[k].started.vw != p.vw || e[k].started.wm != p.wm) p.foreign++;
    }
  }
  return p;
}

static std::string list_text(const std::vector<int> &v)
{
  if (v.empty()) return "-";
  std::string s;
  for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
  return s;
}

static void run_case(const std::vector<ManyEntry> &e)
{
  const int n = (int)e.size();
  const ManyPlan p = many_shape_decide(e.empty() ? nullptr : e.data(), n);
  if (p.rc) {
    CHECK(p.rc == MPF_E_STATE && !p.error.empty(), "an error without a message (rc %d)", p.rc);
    CHECK(p.batch.empty() && p.alone.empty(), "an error with a plan");
  } else {
    std::vector<int> seen((size_t)n, 0);
    int last = -1;
    for (int k : p.batch) {
      CHECK(k > last && k < n, "batch not ascending at %d", k);
      last = k;
      seen[(size_t)k]++;
      const ManyShape &own = e[(size_t)k].state == 2 ? e[(size_t)k].started : e[(size_t)k].now;
      CHECK(own == p.shape, "engine %d (%s) in a launch on %s", k, many_shape_text(own).c_str(), many_shape_text(p.shape).c_str());
      CHECK(e[(size_t)k].state == 2 || e[(size_t)k].fits, "engine %d does not fit the batch", k);
      CHECK(p.shape.vw > 0, "a launch without a width");
    }
    last = -1;
    for (int k : p.alone) {
      CHECK(k > last && k < n, "alone not ascending at %d", k);
      last = k;
      seen[(size_t)k]++;
      CHECK(e[(size_t)k].state == 1, "engine %d runs alone in state %d", k, (int)e[(size_t)k].state);
    }
    for (int k = 0; k < n; k++) CHECK(seen[(size_t)k] == (e[(size_t)k].state ? 1 : 0), "engine %d placed %d times", k, seen[(size_t)k]);
  }
  const ParentPlan q = parent_rule(e);
  std::printf("case %d rc %d vw %d S %d wm %d dev %d batch %s alone %s owner %d | parent vw %d batch %s foreign %d%s%s\n", g_case, p.rc, p.batch.empty() ? 0 : p.shape.vw,
              p.batch.empty() ? 0 : p.shape.S, (p.batch.empty() || !p.shape.wm) ? 0 : 1, p.batch.empty() ? 0 : p.shape.dev, list_text(p.batch).c_str(),
              list_text(p.alone).c_str(), p.batch.empty() ? -1 : p.batch[0], q.vw, list_text(q.batch).c_str(), q.foreign, p.rc ? " | " : "", p.error.c_str());
}

int main(int argc, char **argv)
{
  if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    long n = -1;
    if (!(ls >> n) || n < 0 || n > 100000) { std::fprintf(stderr, "bad case line\n"); return 2; }
    std::vector<ManyEntry> e((size_t)n);
    for (auto &t : e) {
      long v[12];
      for (long &x : v) if (!(ls >> x)) { std::fprintf(stderr, "short case line\n"); return 2; }
      t.state = (uint8_t)v[0];
      t.now.vw = (int)v[1]; t.now.S = (int)v[2]; t.now.dev = (int)v[3]; t.now.wm = v[4] != 0;
      t.pack_gen = (uint64_t)v[5];
      t.fits = v[6] != 0;
      t.started.vw = (int)v[7]; t.started.S = (int)v[8]; t.started.dev = (int)v[9]; t.started.wm = v[10] != 0;
      t.started_gen = (uint64_t)v[11];
    }
    run_case(e);
    g_case++;
  }
  return 0;
}
