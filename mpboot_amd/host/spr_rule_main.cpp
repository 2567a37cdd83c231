// spr_rule_main.cpp -- the SPR decision rules of spr_rule.hpp as a stand-alone program: no device, no engine.
// tests/test_spr_rule_host.py builds it with -fsanitize=address,undefined, runs it as a child process and compares every line
// of its output with a Python restatement of the reference's two rules.
//
// stdin:   tie_mode seed best randomMP n_visits
//          then per visit:  have_move k cost_1 .. cost_k        (k may be 0)
// A visit runs as one prune-node visit of the sweep loop: under MPF_TIE_RANDOM the hits start at 1, every cost is offered to the
// tie rule in order, then the accept rule; an accepted move makes best the current tree's length (randomMP).
// stdout:  per visit  "taken best hits iter_hits accept state"  -- taken: the number of the candidate selected last (-1: none),
//          state: the generator's state behind the visit (hex), i.e. how many draws have been taken.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "rng.hpp"
#include "spr_rule.hpp"

using namespace mpf;

int main()
{
  int tie_mode = 0, seed = 0, n_visits = 0;
  uint32_t best = 0, randomMP = 0;
  if (std::scanf("%d %d %" SCNu32 " %" SCNu32 " %d", &tie_mode, &seed, &best, &randomMP, &n_visits) != 5 || n_visits < 0) return 2;
  if (tie_mode != MPF_TIE_FIRST && tie_mode != MPF_TIE_RANDOM) return 2;
  TieRng rng;
  rng.seed(seed);
  auto draw = [&] { return rng.next(); };
  unsigned long hits = 1;
  unsigned iter_hits = 1;
  std::vector<uint32_t> cost;
  for (int v = 0; v < n_visits; v++) {
    int have_move = 0, k = 0;
    if (std::scanf("%d %d", &have_move, &k) != 2 || k < 0 || k > (1 << 20)) return 2;
    cost.resize((size_t)k);
    for (uint32_t &c : cost)
      if (std::scanf("%" SCNu32, &c) != 1) return 2;
    if (tie_mode == MPF_TIE_RANDOM) hits = 1;
    long taken = -1;
    for (int c = 0; c < k; c++)
      if (sprrule::offer(tie_mode, cost[(size_t)c], best, hits, draw)) taken = c;
    const bool accept = sprrule::accept(tie_mode, best, randomMP, iter_hits, have_move != 0, draw);
    if (accept) randomMP = best;
    std::printf("%ld %" PRIu32 " %lu %u %d %016" PRIx64 "\n", taken, best, hits, iter_hits, (int)accept, rng.state);
  }
  return 0;
}
