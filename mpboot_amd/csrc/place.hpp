// place.hpp -- launch interface of the taxon-insertion kernels (place.hip; host/place.cpp).
//
// addTaxonMPFast (phylotree.cpp:1322-1378) tries a taxon on every branch of a tree; the length of the tree with query tip T in
// the middle of a branch whose two directed views are A and B is len(tree) + #sites where X and T share no state, X = A & B where
// that is non-empty, else A | B.  For Q queries and B branches that is a Q x B x row-words popcount product.
#pragma once
#include "kernels.hpp"

namespace mpf {

// Tile shapes of k_place_costs (compile-time).  A workgroup of 256 lanes owns TQ queries x TB branches and walks the
// row in slices of KS words; a lane holds RQ x RB outputs and, in the narrow shape, one of KT interleaved word classes of a slice
// (summed through LDS at the end: no atomics).
//   wide   (many queries):  4 rows: 64 x 64, 4 x 4 per lane, KS 16;   20 | 32 rows: 32 x 32, 2 x 2 per lane, KS 4
//   narrow (few outputs, every computeParsimonyTree step): 4 queries x 16 branches, 4 x 1 per lane, KT = KS = 16
enum { PLACE_AUTO = 0, PLACE_NARROW = 1, PLACE_WIDE = 2 };
struct PlaceShape { int tq, tb, ks; };
PlaceShape place_shape(int S, int tile);            // tile: PLACE_NARROW | PLACE_WIDE
int place_pick(int n_query, int n_br, int tile);    // PLACE_AUTO -> the shape for that many outputs (narrow below 2^18)

// delta[q * ld + b] = #sites (weight-replicated) at which branch b = (desc[b].a, desc[b].b: slots of its two directed views, a
// tip's own vector at a pendant branch) joined as above shares no state with the vector in slot qslot[q].  Row-major store only.
hipError_t launch_place_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br,
                              const uint32_t *qslot, int n_query, uint32_t *delta, int ld, int tile);
// best[2 q] = min_b delta[q * ld + b], best[2 q + 1] = the lowest b that has it (one wave per query)
hipError_t launch_place_best(hipStream_t st, const uint32_t *delta, int n_br, int n_query, int ld, uint32_t *best);

// my_random_shuffle over the identity on the stream handed over by state (placetree::shuffle_order, host/place_tree.hpp)
void place_shuffle_order(int n, uint64_t *state, int32_t *order);

}  // namespace mpf
