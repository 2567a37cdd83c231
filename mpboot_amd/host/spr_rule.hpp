// spr_rule.hpp -- the two rules an SPR hill climb decides by, device-free: no HIP, no engine.  Every host loop that takes such
// a decision (host/search.cpp, the tracked climbs through host/ufboot_common.hpp, the per-sample replay of host/ufboot_refine.cpp)
// calls these; spr_rule_main.cpp runs them alone.  `draw` is a callable returning the next random_double(): the number of calls
// is part of the rule -- every draw of a climb comes from one stream.
#pragma once
#include <cstdint>
#include "../../include/mpfitch.h"

namespace mpf {
namespace sprrule {

// testInsertParsimony's tie rule for one candidate of length mp (sprparsimony.cpp:2168-2176; stepwise addition :3001-3008):
// best = bestParsimony, hits = bestTreeScoreHits.  A longer candidate changes nothing and draws nothing; an equally long one
// counts a hit and draws against 1 / hits (MPF_TIE_FIRST: it is no candidate); a shorter one is taken without a draw and, under
// MPF_TIE_RANDOM, starts the hits again.  True if the candidate was taken (best == mp then).
template <class Count, class Draw>
inline bool offer(int tie_mode, uint32_t mp, uint32_t &best, Count &hits, Draw &&draw)
{
  if (mp > best) return false;
  if (mp < best) {
    if (tie_mode == MPF_TIE_RANDOM) hits = 1;
    best = mp;
    return true;
  }
  if (tie_mode != MPF_TIE_RANDOM) return false;
  hits++;
  return draw() <= 1.0 / (double)hits;
}

// The sweep's accept rule behind one prune-node visit (sprparsimony.cpp:3306-3311): iter_hits = bestIterationScoreHits,
// randomMP = the current tree's length, have_move = removeNode && insertNode.  A visit that ends level with the current tree
// counts a hit and draws -- also when it selected nothing: the move test comes behind the draw.
template <class Count, class Draw>
inline bool accept(int tie_mode, uint32_t best, uint32_t randomMP, Count &iter_hits, bool have_move, Draw &&draw)
{
  if (tie_mode != MPF_TIE_RANDOM) return best < randomMP;
  if (best < randomMP) {
    iter_hits = 1;
    return have_move;
  }
  if (best > randomMP) return false;
  iter_hits++;
  return draw() <= 1.0 / (double)iter_hits && have_move;
}

}  // namespace sprrule
}  // namespace mpf
