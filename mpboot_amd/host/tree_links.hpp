// tree_links.hpp -- one walk over a record-format tree: the check of its back links and the layout of the topology array the
// device reads, free of any device code.
//
// A complete tree of n taxa has the nodes 1 .. 2n - 2; node v owns the records 3v, 3v + 1, 3v + 2 (a tip uses the first only) and
// back[r] is the record at the far end of r's branch.  A vector slot per record: tip v -> v - 1, record 3v + s of an inner node
// -> n + 3 (v - n - 1) + s.  kids[slot r] = the slots of the two records behind r, in `next` order: what a refresh combines into
// r's vector and what a scan descends into.
//
// Engine::set_tree checks a tree handed over (no output array); Engine::schedule_views_dev lays out the tree the engine holds,
// straight into the pinned stage the copy kernel reads (no check: that tree has passed it).
// tests/cpu/tree_links_test.cpp compiles this header with g++ -fsanitize=address,undefined.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mpf {
namespace links {

// what mpf_set_tree says of a tree that fails the check
inline const char *bad_links_message() { return "mpf_set_tree: inconsistent back links"; }

inline uint32_t slot_of(int r, int n_taxa)
{
  const int v = r / 3;
  return v <= n_taxa ? (uint32_t)(v - 1) : (uint32_t)(n_taxa + 3 * (v - n_taxa - 1) + r % 3);
}

// back: 3 (2n - 1) entries.  Every record in use must link to a record b with 3 <= b < 3 (2n - 1) that links back; false at the
// first one that does not (kids is then written in part: a caller hands over scratch, never the array it relies on).
// kids (Pair: two 32-bit members x, y; nullptr: the check alone): n + 3 (n - 2) entries, of which those of the inner records are
// written -- the three of a node side by side.
// Check = false: the links are known to be good (a tree that passed, or one the engine built): the layout alone, without the
// dependent load behind every link.
template <typename Pair, bool Check = true>
inline bool check_and_layout(int n_taxa, const int32_t *back, Pair *kids)
{
  const int len = 3 * (2 * n_taxa - 1);
  if (Check)
    for (int v = 1; v <= n_taxa; v++) {
      const int r = 3 * v, b = back[r];
      if (b < 3 || b >= len || back[b] != r) return false;
    }
  for (int v = n_taxa + 1; v <= 2 * n_taxa - 2; v++) {
    const int r0 = 3 * v;
    uint32_t s[3];
    for (int k = 0; k < 3; k++) {
      const int b = back[r0 + k];
      if (Check && (b < 3 || b >= len || back[b] != r0 + k)) return false;
      s[k] = slot_of(b, n_taxa);
    }
    if (kids) {
      Pair *k = kids + (n_taxa + 3 * (v - n_taxa - 1));
      k[0].x = s[1]; k[0].y = s[2];
      k[1].x = s[2]; k[1].y = s[0];
      k[2].x = s[0]; k[2].y = s[1];
    }
  }
  return true;
}

}  // namespace links
}  // namespace mpf
