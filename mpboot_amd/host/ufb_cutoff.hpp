// ufb_cutoff.hpp -- the cut-off filter of IQTree::saveCurrentTree, device-free: no HIP, no engine.  Every loop that books trees
// under -bb (the tracked SPR loops, the tracked NNI steps, the quiet stretch of a climb) takes its limits and both of its tests
// from here; ufb_cutoff_main.cpp runs them alone.
#pragma once
#include <cmath>
#include <cstdint>

namespace mpf {

// A tree of length len is saved iff  -len > logl_cutoff - 1e-4  (iqtree.cpp:3343), i.e. len < lim = -logl_cutoff + 1e-4:
// mp_max = the largest length that passes, none_pass = no length does.  logl_cutoff == 0.0: no cut-off in force.
struct UfbCutoff {
  bool have_cut = false, none_pass = false;
  uint32_t mp_max = UINT32_MAX;
  // the rule of iqtree.cpp:3343 for one tree
  bool passes(uint32_t len) const { return len <= mp_max && !none_pass; }
  // for the candidates of a part whose costs count from `base`: cost < threshold <=> base + cost <= mp_max (0: none of them;
  // saturated where mp_max - base + 1 does not fit: no cost reaches 2^32 - 1).  With none_pass nothing is multiplied at all.
  uint32_t part_threshold(uint32_t base) const
  {
    if (mp_max < base) return 0u;
    return mp_max - base == UINT32_MAX ? UINT32_MAX : mp_max - base + 1u;
  }
};

inline UfbCutoff ufb_cutoff(double logl_cutoff)
{
  UfbCutoff c;
  if (logl_cutoff == 0.0) return c;
  c.have_cut = true;
  const double lim = -logl_cutoff + 1e-4;
  c.none_pass = !(lim > 0.0);
  if (c.none_pass) c.mp_max = 0u;
  else {
    const double top = std::ceil(lim) - 1.0;       // (a cut-off below -2^32: every length a word holds passes)
    c.mp_max = top >= 4294967295.0 ? UINT32_MAX : (uint32_t)top;
  }
  return c;
}

}  // namespace mpf
